"""Points in boxes without a GPU: the host entry point (vg_points_in_boxes_host runs the kernel's own per-pair code,
csrc/points_in_boxes_pair.inc) against the 60-digit fixture of tests/golden/make_points_in_boxes.py on EVERY point of families A-D,
FrameState.set_proposals and get_box_heights against the reference's own run (family E), and every argument error.

THE TIE ZONE (family B).  The fixture decides the rule exactly; the kernel decides it in float64.  The two can differ only for a
point whose exact lx or ly lies closer to its face than the kernel's error in that value, so the generator emits no such point.  The
error, with u = 2^-53 and the stored inputs exact (float32 points widened, boxes in their dtype, the faces dx / 2 + 1e-5 and
dy / 2 + 1e-5 the float64 values the rule names):
    sx = fl(x - cx), sy = fl(y - cy)            one rounding each:             <= u |sx|, u |sy|
    cs, sn = iou_sincos(rz)                     below an ulp of a value <= 1:   <= 2 u each        (csrc/iou_pair.inc: < 1 ulp)
    sx cs, sy sn                                one rounding each:             <= u |sx|, u |sy|
    lx = fl(. + .)                              one rounding of |lx| <= |sx| + |sy|
so  |lx_kernel - lx|  <=  (1 + 2 + 1 + 1) u (|sx| + |sy|)  =  5 u (|sx| + |sy|)  to first order, and the same for ly; the second-order
terms are below u^2 x 10 (|sx| + |sy|).  The generator takes TIE_UNITS = 6 for the 5 (+ second order) and keeps every point of
family B at least 8 x 6 u (|sx| + |sy|) from both faces of every box it is tested against -- it asserts so when it runs and stores the
smallest distance it met in units of that bound (`B_min_clearance`, asserted > 1 here; 2.6e4 in the committed file).  At these
centres (|sx| + |sy| < 10) the bound is ~5e-14 and a float32 step is >= 1e-6, so nothing had to be left out: every generated point
is in the file and the tests exclude none.
Family A (heading exactly 0): iou_sincos(0) = (0, 1) exactly, the differences of a float32 and an integer centre are exact, sx * 1 +
sy * 0 is exact: the kernel's arithmetic IS the rule, the equality cases included.  The z test is one exact difference in every family.
"""
import ctypes

import numpy as np
import pytest

import pib_ref as R
from vilgod_amd import build, points_in_boxes as pib
from vilgod_amd._lib import lib, parse_header, VilgodHipError
from vilgod_amd.frame_state import FrameState, INDEX_ALL_POINTS, INDEX_WO_GROUND


@pytest.fixture(scope='module')
def g():
    return R.fixture()


def test_header_declares_and_library_exports_the_entries():
    protos = parse_header()
    assert len(protos['vg_points_in_boxes'][1]) == 9 and len(protos['vg_points_in_boxes_host'][1]) == 8
    assert lib.vg_points_in_boxes and lib.vg_points_in_boxes_host
    assert lib.vg_abi_version() == 2                                   # an addition: the version stays
    assert pib.PIB_CHUNK == 256
    assert build.SOURCES['points_in_boxes.hip'] == ['-ffp-contract=off']


def test_kernel_is_built_without_scratch_and_without_unencodable_constants():
    assert build.check_scratch('points_in_boxes.hip', 'k_points_in_boxes') == []
    import re
    text = build._device_asm('points_in_boxes.hip')
    assert len(re.findall(r'^_Z17k_points_in_boxesI[fd]E\S*:', text, flags=re.M)) == 2          # both box dtypes are there
    assert not re.search(r's_mov_b64\s+s\[[0-9:]+\],\s*0x[0-9a-fA-F]{9,}', text)                # build.check_isa's pattern


@pytest.mark.parametrize('family', R.FAMILIES)
def test_host_entry_point_equals_the_fixture_on_every_point(g, family):
    pts, boxes, want = g[f'{family}_points'], g[f'{family}_boxes'], g[f'{family}_expect']
    assert boxes.dtype == (np.float32 if family.endswith('32') else np.float64) and pts.dtype == np.float32
    got = R.host_batched(pts, boxes)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (family, len(bad), bad[:5], got[got != want][:5], want[got != want][:5])
    assert np.any(want >= 0) and np.any(want < 0)
    if family[0] == 'C':
        assert want.max() >= 2 and np.any(want[0] != want[1])          # the reversed order gives other winners
    if family[0] == 'D':
        # nothing is inside a box with a negative extent, a NaN or |rz| = 2e6; the zero extents and the sound box own points
        assert set(np.unique(want).tolist()) == {-1, 0, 1, 2, 17}


def test_fixture_keeps_the_tie_zone_clear(g):
    assert g['B_min_clearance'] > 1.0 and int(g['tie_units']) == 6 and int(g['tie_margin']) == 8


def test_python_form_is_the_batched_entry_point_one_set_at_a_time(g):
    for family in ('A32', 'B32', 'C32', 'D32'):
        for s in range(len(g[f'{family}_points'])):
            got = pib.points_in_boxes_host(g[f'{family}_points'][s], g[f'{family}_boxes'][s])
            assert got.dtype == np.int64 and np.array_equal(got, g[f'{family}_expect'][s])
    # float64 input is cast to float32 as pointcloud_utils.py:518-520 does; extra columns are ignored
    pts, boxes = g['C32_points'][0], g['C32_boxes'][0]
    wide_p = np.c_[pts.astype(np.float64), np.full((len(pts), 2), 7.0)]
    wide_b = np.c_[boxes.astype(np.float64), np.full((len(boxes), 2), 7.0)]
    assert np.array_equal(pib.points_in_boxes_host(wide_p, wide_b), g['C32_expect'][0])


def test_no_boxes_and_no_points(g):
    pts = g['C32_points'][0]
    assert np.array_equal(pib.points_in_boxes_host(pts, np.zeros((0, 7))), np.full(len(pts), -1))
    assert pib.points_in_boxes_host(np.zeros((0, 3)), g['C32_boxes'][0]).shape == (0,)
    assert np.array_equal(R.host_batched(g['C64_points'], np.zeros((2, 0, 7))), np.full((2, len(pts)), -1))


def test_stride_and_batch_layout(g):
    pts, boxes, want = g['B64_points'], g['B64_boxes'], g['B64_expect']
    wide = np.full(pts.shape[:2] + (5,), 1e6, np.float32)
    wide[:, :, :3] = pts
    assert np.array_equal(R.host_batched(wide, boxes), want)
    # each set alone gives its row of the batch
    for s in (0, len(pts) - 1):
        assert np.array_equal(R.host_batched(pts[s:s + 1], boxes[s:s + 1])[0], want[s])


# ---- family E: the reference's generate_detections(None, proposals=..., names=...) and get_box_heights --------------------------------
def _frame_state(g, with_names=True):
    from vilgod_amd.sequence_datasets import apply_transform
    fs = FrameState(2, g['E_pose'], g['E_ref_pose'])
    pts = g['E_points']
    ref = apply_transform(pts, fs.transform_to_ref)
    props_ref = apply_transform(g['E_proposals'], fs.transform_to_ref, box=True)
    idx = pib.points_in_boxes_host(ref, props_ref)
    fs.set_proposals(props_ref, idx, g['E_names'] if with_names else None)
    return fs, props_ref, idx


def test_set_proposals_reproduces_the_reference_detections(g):
    fs, props_ref, idx = _frame_state(g)
    assert fs.index_space == INDEX_ALL_POINTS
    assert np.array_equal(fs.cluster_ids, g['E_cluster_id']) and fs.cluster_ids.tolist() == [0, 1, 2, 3, 5, 6, 7]     # 4 owns no point
    assert np.array_equal(fs.seg_off, g['E_seg']) and np.array_equal(fs.index, g['E_index'])
    dets = fs.serialize['_detections']
    assert len(dets) == len(g['E_cluster_id'])
    for c, d in enumerate(dets):
        assert d['cluster_id'] == g['E_cluster_id'][c]
        assert np.array_equal(d['cluster_points_index'], g['E_index'][g['E_seg'][c]:g['E_seg'][c + 1]])
        assert np.array_equal(d['cluster_points_index'], np.flatnonzero(idx == d['cluster_id']))              # ascending, all points
        assert d['_bounding_box'].dtype == np.float64 and np.array_equal(d['_bounding_box'], g['E_box'][c])
        assert np.array_equal(d['_bounding_box'], props_ref[d['cluster_id'], :7])
        assert dict(d['object_class']) == {'proposal': g['E_object_class'][c]}
        assert list(d) == ['cluster_id', '_bounding_box', 'valid', 'static', 'gt_assigned', 'cluster_points_index', 'tid', 'object_class']
    # the frame survives its own serialisation, and a compact copy serialises alike
    back = FrameState(2, g['E_pose'], g['E_ref_pose'])
    back.sync(fs.serialize)
    again = back.serialize['_detections']
    assert [dict(d['object_class']) for d in again] == [dict(d['object_class']) for d in dets]
    assert all('object_class_score' not in d and 'object_class_predictions' not in d for d in again)
    compact = FrameState.from_compact(fs.compact()).serialize['_detections']
    assert [list(d) for d in compact] == [list(d) for d in dets]


def test_set_proposals_without_names_and_with_packed_lists(g):
    fs, props_ref, idx = _frame_state(g, with_names=False)
    assert all('object_class' not in d for d in fs.serialize['_detections'])
    from vilgod_amd.frame_state import pack_clusters
    other = FrameState(2, g['E_pose'], g['E_ref_pose'])
    other.set_proposals(props_ref, pack_clusters(idx, None, 0.0), g['E_names'])
    assert np.array_equal(other.index, fs.index) and np.array_equal(other.seg_off, fs.seg_off) and np.array_equal(other.cluster_ids, fs.cluster_ids)
    empty = FrameState(2, g['E_pose'], g['E_ref_pose'])
    empty.set_proposals(np.zeros((0, 7)), np.full(100, -1), None)
    assert empty.n_detections == 0 and empty.serialize['_detections'] == [] and empty.index_space == INDEX_ALL_POINTS


def test_a_stage_that_reads_points_without_ground_refuses_a_proposal_frame(g):
    fs, _, _ = _frame_state(g)
    with pytest.raises(ValueError, match='points_ref_wo_ground'):
        fs.require_index_space(INDEX_WO_GROUND, 'the box fit')
    fs.require_index_space(INDEX_ALL_POINTS, 'label_proposals')
    plain = FrameState(0, np.eye(4), np.eye(4))
    plain.set_clusters(np.array([3], np.int64), np.array([0, 1], np.int32), np.array([0, 2], np.int32))
    plain.require_index_space(INDEX_WO_GROUND, 'the box fit')
    with pytest.raises(ValueError, match='points_ref'):
        plain.require_index_space(INDEX_ALL_POINTS, 'label_proposals')
    fs.set_clusters(np.array([3], np.int64), np.array([0, 1], np.int32), np.array([0, 2], np.int32))             # clusters again: back to the default
    assert fs.index_space == INDEX_WO_GROUND


def test_get_box_heights_with_host_membership(g):
    pts, props = g['E_points'], g['E_proposals']
    got = pib.get_box_heights(pts, props, membership=pib.points_in_boxes_host)
    assert got.dtype == props.dtype and np.array_equal(got, g['E_heights'])
    assert np.array_equal(got[4], props[4]) and not np.array_equal(got[0], props[0])                            # the empty box is unchanged
    assert np.array_equal(got[:, [0, 1, 3, 4, 6]], props[:, [0, 1, 3, 4, 6]])


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_every_value_error_names_its_argument():
    import torch
    p2, b2 = np.zeros((4, 3), np.float32), np.zeros((2, 7), np.float32)
    for fn in (pib.points_in_boxes_host, pib.points_in_boxes):
        with pytest.raises(ValueError, match='points'):
            fn(np.zeros((1, 4, 3)), b2)
        with pytest.raises(ValueError, match='points'):
            fn(np.zeros((4, 2)), b2)
        with pytest.raises(ValueError, match='boxes'):
            fn(p2, np.zeros(7))
        with pytest.raises(ValueError, match='boxes'):
            fn(p2, np.zeros((2, 6)))
    with pytest.raises(ValueError, match='boxes'):
        pib.get_box_heights(p2, np.zeros((2, 6)), membership=pib.points_in_boxes_host)
    tp, tb = torch.zeros((1, 4, 3)), torch.zeros((1, 2, 7))
    with pytest.raises(ValueError, match='points'):
        pib.points_in_boxes_gpu(tp, tb)                               # CPU tensors
    with pytest.raises(ValueError, match='points'):
        pib.points_in_boxes_gpu(p2, tb)                               # not a tensor
    with pytest.raises(ValueError, match='points'):
        pib.points_in_boxes_gpu(tp[0], tb)
    with pytest.raises(ValueError, match='points'):
        pib.points_in_boxes_gpu(tp[:, :, :2], tb)
    with pytest.raises(ValueError, match='points'):
        pib.points_in_boxes_gpu(tp.double(), tb)
    with pytest.raises(ValueError, match='boxes'):
        pib.points_in_boxes_gpu(tp, tb[0])
    with pytest.raises(ValueError, match='boxes'):
        pib.points_in_boxes_gpu(tp, tb[:, :, :6])
    with pytest.raises(ValueError, match='boxes'):
        pib.points_in_boxes_gpu(tp, tb.half())
    with pytest.raises(ValueError, match='batch'):
        pib.points_in_boxes_gpu(tp, torch.zeros((2, 2, 7)))
    fs = FrameState(0, np.eye(4), np.eye(4))
    with pytest.raises(ValueError, match='proposals_ref'):
        fs.set_proposals(np.zeros((3, 6)), np.zeros(5, np.int64))
    with pytest.raises(ValueError, match='box_idx'):
        fs.set_proposals(np.zeros((3, 7)), np.zeros((5, 1), np.int64))
    with pytest.raises(ValueError, match='box_idx'):
        fs.set_proposals(np.zeros((3, 7)), np.array([0, 3, -1]))
    with pytest.raises(ValueError, match='names'):
        fs.set_proposals(np.zeros((3, 7)), np.array([0, 2, -1]), names=['a', 'b'])


def test_every_bad_argument_of_the_c_entry_points_is_refused():
    pts = np.zeros((6, 3), np.float32)
    boxes = np.zeros((2, 7), np.float64)
    boxes[:, 3:6] = 1.0
    out = np.full(6, -7, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def host(dtype=1, p=P(pts), stride=3, n=6, b=P(boxes), m=2, batch=1, o=P(out)):
        return lib.vg_points_in_boxes_host(dtype, p, stride, n, b, m, batch, o)

    def device(dtype=1, p=P(pts), stride=3, n=6, b=P(boxes), m=2, batch=1, o=P(out)):
        return lib.vg_points_in_boxes(dtype, p, stride, n, b, m, batch, o, None)

    # (the device entry point checks its arguments before it touches the runtime: none of these calls launches anything)
    for call in (host, device):
        assert call(dtype=2) == 1 and call(dtype=-1) == 1
        assert call(stride=2) == 1 and call(stride=0) == 1
        assert call(n=-1) == 1 and call(m=-1) == 1 and call(batch=-1) == 1
        assert call(p=None) == 1 and call(o=None) == 1 and call(b=None) == 1
        assert call(n=0, p=None, o=None, b=None) == 0 and call(batch=0, p=None, o=None, b=None) == 0
    assert np.all(out == -7)
    assert host() == 0 and np.array_equal(out, [0] * 6)
    assert host(b=None, m=0) == 0 and np.array_equal(out, [-1] * 6)          # no boxes: -1 everywhere, the box pointer may be null
    assert device(batch=65536) == 3
