"""The rotated-box IoU (csrc/iou.hip) on the CPU, through vg_boxes_iou3d_host and so through the shipped pair body
(csrc/iou_pair.inc), against the 60-digit reference of tests/golden/make_iou.py.

The bar is stated and derived in tests/iou_ref.py: per pair min(max(8 * E_host[family], 2^-50), 2^-50 + 2^-44 R^2 / U), E_host (host
numpy iou3d_matrix against the same reference, measured by the generator) = 5.551e-16 / 4.286e-10 / 4.286e-10 / 2.776e-16 / 3.343e-14
for the families A .. E.  The share of the bar each family uses is printed (`pytest -s`)."""
import ctypes
import os

import numpy as np
import pytest

import iou_ref as R
from conftest import ROOT
from vilgod_amd import evaluation as ev, iou

VG_ERR_ARG = 1


@pytest.fixture(scope='module')
def g():
    return R.fixture()


@pytest.fixture(scope='module')
def host_values(g):
    """the host entry point on every fixture pair, one group per pair, computed once: {mode: [P]}"""
    off = R.one_group_per_pair(len(g['a']))
    return {mode: iou.iou_groups_host(g['a'], off, g['b'], off, mode)[0] for mode in (0, 1, 2)}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _raw(a, a_off, b, b_off, out_off, out, mode=0, dtype=1):
    from vilgod_amd._lib import lib
    a_off, b_off, out_off = np.ascontiguousarray(a_off, np.int32), np.ascontiguousarray(b_off, np.int32), np.ascontiguousarray(out_off, np.int64)
    return lib.vg_boxes_iou3d_host(dtype, _p(a), _p(a_off), _p(b), _p(b_off), len(a_off) - 1, _p(out_off), mode, _p(out))


def test_fixture_is_what_the_generator_promises(g):
    fam = g['family']
    assert [int((fam == k).sum()) for k in range(5)] == [92, 440, 2220, 72, 2000]
    assert set(g['n_vert'][fam == 3].tolist()) >= {3, 4, 5, 6, 7, 8}
    assert np.mean(g['ref'][fam == 4, 2] > 0) >= 0.5
    c = fam == 2
    assert np.all(fam[g['twin'][c]] != 2) and np.all(g['twin'][~c] == -1)
    assert np.allclose(g['e_host'], [5.551e-16, 4.286e-10, 4.286e-10, 2.776e-16, 3.343e-14], rtol=1e-3)


def test_every_family_meets_the_bar(g, host_values):
    R.check_against_bar(g, host_values, 'host')


def test_float32_input_equals_float64_input_of_the_widened_values(g):
    sel = np.flatnonzero(np.isin(g['family'], (0, 1, 3)))
    a32, b32 = g['a'][sel].astype(np.float32), g['b'][sel].astype(np.float32)
    off = R.one_group_per_pair(len(sel))
    for mode in (0, 1, 2):
        narrow, _ = iou.iou_groups_host(a32, off, b32, off, mode)
        wide, _ = iou.iou_groups_host(a32.astype(np.float64), off, b32.astype(np.float64), off, mode)
        assert narrow.tobytes() == wide.tobytes()
    assert np.any(narrow > 0)


def test_a_pairs_bits_do_not_depend_on_companions_position_or_group_order(g, host_values):
    rng = np.random.default_rng(5)
    sel = rng.choice(len(g['a']), 240, replace=False)
    a, b = g['a'][sel], g['b'][sel]
    alone = host_values[0][sel]
    # companions: the full 240 x 240 matrix holds every pair on its diagonal
    full, _ = iou.iou_groups_host(a, [0, 240], b, [0, 240])
    assert np.diagonal(full.reshape(240, 240)).tobytes() == alone.tobytes()
    # position: groups of uneven sizes, the pair (i, i) sits somewhere inside its group's matrix
    cuts = np.array([0, 1, 3, 3, 40, 41, 120, 240])
    grouped, out_off = iou.iou_groups_host(a, cuts, b, cuts)
    for k in range(len(cuts) - 1):
        n = cuts[k + 1] - cuts[k]
        m = grouped[out_off[k]:out_off[k] + n * n].reshape(n, n)
        assert np.diagonal(m).tobytes() == alone[cuts[k]:cuts[k + 1]].tobytes()
    # order of groups: the same groups, reversed
    order = np.arange(len(cuts) - 1)[::-1]
    ra = np.concatenate([a[cuts[k]:cuts[k + 1]] for k in order])
    rb = np.concatenate([b[cuts[k]:cuts[k + 1]] for k in order])
    rcuts = np.concatenate([[0], np.cumsum([cuts[k + 1] - cuts[k] for k in order])])
    rev, rev_off = iou.iou_groups_host(ra, rcuts, rb, rcuts)
    for pos, k in enumerate(order):
        n = cuts[k + 1] - cuts[k]
        assert rev[rev_off[pos]:rev_off[pos] + n * n].tobytes() == grouped[out_off[k]:out_off[k] + n * n].tobytes()


def test_shapes_and_empty_groups(g, host_values):
    a, b = g['a'][:12], g['b'][:12]
    for na, nb in ((0, 5), (5, 0), (1, 1)):
        out, off = iou.iou_groups_host(a[:na], [0, na], b[:nb], [0, nb])
        assert out.shape == (na * nb,) and off.tolist() == [0]
    assert out[0] == host_values[0][0]
    # seven groups, empty ones first, in the middle and last
    a_off, b_off = [0, 0, 2, 5, 5, 5, 9, 9], [0, 3, 4, 7, 7, 9, 12, 12]
    out, off = iou.iou_groups_host(a, a_off, b, b_off)
    sizes = np.diff(a_off) * np.diff(b_off)
    assert sizes.tolist() == [0, 2, 9, 0, 0, 12, 0] and len(out) == 23
    for k in range(7):
        want, _ = iou.iou_groups_host(a[a_off[k]:a_off[k + 1]], [0, a_off[k + 1] - a_off[k]], b[b_off[k]:b_off[k + 1]], [0, b_off[k + 1] - b_off[k]])
        assert out[off[k]:off[k] + sizes[k]].tobytes() == want.tobytes()
    # 1000 groups of 1 x 1
    off = R.one_group_per_pair(1000)
    start = int(np.flatnonzero(g['family'] == 4)[0])
    out, _ = iou.iou_groups_host(g['a'][start:start + 1000], off, g['b'][start:start + 1000], off)
    assert out.tobytes() == host_values[0][start:start + 1000].tobytes() and np.count_nonzero(out) > 400
    assert iou.iou_groups_host(a[:0], [0], b[:0], [0])[0].shape == (0,)           # no group at all


def test_output_outside_the_ranges_stays_untouched(g, host_values):
    a, b = np.ascontiguousarray(g['a'][:6]), np.ascontiguousarray(g['b'][:6])
    out = np.full(64, -7.25)
    out_off = [3, 10, 30]                                          # slack in front, between the groups and behind
    assert _raw(a, [0, 2, 2, 6], b, [0, 3, 5, 6], out_off, out) == 0
    written = np.zeros(64, bool)
    written[3:9] = True
    written[30:34] = True
    assert np.all(out[~written] == -7.25) and np.all(out[written] != -7.25)
    assert out[3] == host_values[0][0]


def test_bad_arguments_are_refused(g):
    a, b = np.ascontiguousarray(g['a'][:4]), np.ascontiguousarray(g['b'][:4])
    out = np.full(16, -1.0)
    assert _raw(a, [0, 4], b, [0, 4], [0], out) == 0
    assert _raw(a, [0, 4], b, [0, 4], [0], out, dtype=2) == VG_ERR_ARG
    assert _raw(a, [0, 4], b, [0, 4], [0], out, dtype=-1) == VG_ERR_ARG
    assert _raw(a, [0, 4], b, [0, 4], [0], out, mode=3) == VG_ERR_ARG
    assert _raw(a, [0, 4], b, [0, 4], [0], out, mode=-1) == VG_ERR_ARG
    before = out.copy()
    assert _raw(a, [0, 3, 2, 4], b, [0, 1, 2, 4], [0, 3, 3], out) == VG_ERR_ARG           # a_off falls
    assert _raw(a, [0, 2, 4], b, [0, 3, 2], [0, 6], out) == VG_ERR_ARG                    # b_off falls
    assert _raw(a, [0, 2, 4], b, [0, 2, 4], [4, 0], out) == VG_ERR_ARG                    # out_off falls
    assert _raw(a, [0, 2, 4], b, [0, 2, 4], [0, 3], out) == VG_ERR_ARG                    # ranges overlap
    assert _raw(a, [0, 2, 4], b, [0, 2, 4], [-1, 4], out) == VG_ERR_ARG
    assert _raw(None, [0, 4], b, [0, 4], [0], out) == VG_ERR_ARG                          # null boxes with work to do
    assert _raw(a, [0, 4], b, [0, 4], [0], None) == VG_ERR_ARG
    assert np.array_equal(out, before)
    assert _raw(None, [0, 0], None, [0, 0], [0], None) == 0                               # nothing to do: nothing read
    from vilgod_amd._lib import lib
    assert lib.vg_boxes_iou3d_host(1, None, None, None, None, 0, None, 0, None) == 0
    assert lib.vg_boxes_iou3d_host(1, None, None, None, None, -1, None, 0, None) == VG_ERR_ARG


def test_header_symbols_and_kernel_resources():
    from vilgod_amd import _lib, build
    protos = _lib.parse_header()
    assert len(protos['vg_boxes_iou3d'][1]) == 10 and len(protos['vg_boxes_iou3d_host'][1]) == 9
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'vg_boxes_iou3d') and hasattr(lib, 'vg_boxes_iou3d_host')
    header = open(os.path.join(ROOT, 'include', 'vilgod_hip.h')).read()
    for cite in ('tracking_utils.py:9-20', 'zero_shot_detector.py:737-739', 'waymo_dataset.py:300'):
        assert cite in header
    assert build.SOURCES['iou.hip'] == ['-ffp-contract=off']
    assert build.check_isa(sources=['iou.hip']) == []
    assert build.check_scratch('iou.hip', '') == []


def _metric_args(seed=3):
    return R.scene(seed) + (ev.build_config(difficulties=[1, 2], breakdown_range=True, iou_thresholds=R.SCENE_THRESHOLDS[1:]),)


def test_detection_metrics_switch():
    args = _metric_args()
    with pytest.raises(ValueError):
        ev.detection_metrics(*args, iou='bogus')
    plain, host = ev.detection_metrics(*args), ev.detection_metrics(*args, iou='host')
    assert list(plain) == list(host) and all(plain[k] == host[k] for k in plain)
    assert any(v[0] > 0 for v in plain.values())
    with pytest.raises(ValueError):
        ev.waymo_evaluation([], [], class_name=['Vehicle'], iou='bogus')


def test_scene_seeds_meet_their_conditions():
    """the 20 scenes of test_iou_device.py: with the host IoU every nonzero IoU is at least 1e-6 from its threshold and the best
    assignment leads the second best by at least 1e-6 for every kept set (brute force over all assignments)"""
    cutoffs = ev.build_config()['score_cutoffs']
    assert len(R.SCENE_SEEDS) == 20
    for seed in R.SCENE_SEEDS:
        d_thr, lead = R.scene_margins(seed, ev.iou3d_matrix, cutoffs)
        assert d_thr >= 1e-6 and lead >= 1e-6, (seed, d_thr, lead)
