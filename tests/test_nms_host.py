"""The box NMS (csrc/nms.hip, csrc/nms_pair.inc) through vg_boxes_nms_host, which runs the text the kernels run: keep lists and counts
EQUAL to the numpy greedy reference of tests/nms_ref.py (its pair values are the host IoU pinned to 60-digit arithmetic, or exact
fractions), at the word and wave seams of the device layout, on chains, ties, padding rows, threshold edges and `pre_max`; the Python
call shapes and refusals.  No GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import nms_ref as R
from vilgod_amd import build, iou, nms
from vilgod_amd._lib import lib

MODES = ('rotated', 'normal')


def _check(c, label=''):
    """host == reference, sentinels included -> (keep, counts)"""
    st, keep, counts = R.host_raw(c)
    assert st == 0, label
    w_keep, w_counts = R.reference(c)
    assert np.array_equal(counts, w_counts), (label, counts, w_counts)
    assert np.array_equal(keep, w_keep), (label, np.flatnonzero(keep != w_keep)[:5])
    return keep, counts


def _kept(keep, counts, off, g=0):
    return list(keep[off[g]:off[g] + counts[g]])


# ---- build ---------------------------------------------------------------------------------------------------------------------------
def test_build_flags_and_no_scratch():
    assert build.SOURCES['nms.hip'] == ['-ffp-contract=off']
    assert build.check_scratch('nms.hip', '') == []
    assert nms.MAX_GROUP >= 4096


# ---- seams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_group_sizes_at_the_word_and_wave_seams_in_one_call(mode, dtype):
    c = R.seam_case(mode, dtype, seed=int(dtype == np.float32))
    keep, counts = _check(c, (mode, dtype))
    off = c['off']
    sizes = np.diff(off)
    assert set(sizes) >= {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000} and np.sum(sizes == 1) >= 300
    assert np.all(keep[:off[0]] == R.SENTINEL) and np.all(keep[off[-1]:] == R.SENTINEL) and off[0] > 0 and off[-1] < len(keep)
    assert np.all(counts[sizes == 0] == 0) and np.all(counts[sizes == 1] == 1)
    big = sizes >= 63
    assert np.all(counts[big] > 1) and np.all(counts[big] < sizes[big])           # neither everything nor one row


# ---- the greedy property -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_chain_keeps_the_ends_and_only_the_middle_when_it_leads(mode):
    cs = R.chain_cases(mode)
    for name, c in cs.items():
        keep, counts = _check(c, name)
        chain = {tuple(row) for row in R.CHAIN}
        kept_chain = [tuple(c['boxes'][i]) for i in _kept(keep, counts, c['off']) if tuple(c['boxes'][i]) in chain]
        A, B, C = (tuple(r) for r in R.CHAIN)
        assert kept_chain == ([B] if name == 'chain_b_first' else [A, C]), name
        assert counts[0] == len(c['boxes']) - (2 if name == 'chain_b_first' else 1), name      # the unrelated boxes all stay
    ranks = np.lexsort((np.arange(66), -cs['chain_seam']['scores']))
    assert list(ranks[63:]) == [63, 64, 65]


# ---- order ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_score_order_ties_and_last_bits(mode):
    cs = R.order_cases(mode)
    res = {name: _check(c, name) for name, c in cs.items()}
    for name in ('equal_scores', 'signed_zero'):
        keep, counts = res[name]
        assert keep[0] == 0 and np.all(np.diff(keep[:counts[0]]) > 0), name          # ties go to the lowest row: kept rows ascend
    keep, counts = res['descending']
    assert keep[0] == 0
    keep, counts = res['ascending']
    assert keep[0] == 149 and np.all(np.diff(keep[:counts[0]]) < 0)
    keep, counts = res['last_bit_f32']
    s = cs['last_bit_f32']['scores']
    assert s.dtype == np.float32 and len(set(s)) == 3
    assert np.all(np.diff(s[keep[:counts[0]]].astype(np.float64)) <= 0) and keep[0] == 0
    for name, (keep, counts) in res.items():
        assert 1 < counts[0] < 150, name


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_padding_rows_are_never_kept_and_never_suppress(mode, dtype):
    c, best = R.padding_case(mode, dtype)
    keep, counts = _check(c, (mode, dtype))
    kept = _kept(keep, counts, c['off'])
    assert not set(kept) & {5, 6, 10, 70, 20, 21, 22, 23, 24}
    assert kept[0] == 11                                           # a +inf score is a score and leads
    assert best in kept                                            # its higher-scored duplicate with a NaN heading did not suppress it
    # the same rows without the padding rows: the same keep list
    ok = np.setdiff1d(np.arange(140), [5, 6, 10, 70, 20, 21, 22, 23, 24])
    c2 = R.case(c['boxes'][ok], c['scores'][ok], [0, len(ok)], c['thresh'], mode)
    keep2, counts2 = _check(c2)
    assert list(ok[keep2[:counts2[0]]]) == kept


# ---- threshold edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_threshold_edges_are_strict(mode):
    a, b = R.EDGE[:1], R.EDGE[1:]
    for x, y in ((a, b), (b, a)):
        assert iou.iou_groups_host(x, [0, 1], y, [0, 1], iou.MODE_BEV)[0][0] == 0.5
        assert R.normal_fraction(x[0], y[0]) == Fraction(1, 2)
    cs = R.threshold_cases(mode)
    res = {name: _check(c, name) for name, c in cs.items()}
    for tag, first in (('', 0), ('_swapped', 1)):
        assert _kept(*res['edge_at' + tag], [0, 2]) == [first, 1 - first]            # 0.5 > 0.5 is false: both stay
        assert _kept(*res['edge_below' + tag], [0, 2]) == [first]
    keep, counts = res['duplicates_at_one']
    assert counts[0] == 80                                                           # 1.0 > 1.0 is false
    c = cs['minus_one']
    keep, counts = res['minus_one']
    assert list(counts) == [1, 0, 1]
    assert keep[0] == np.argmax(c['scores'][:30]) and keep[30] == 30 + np.argmax(c['scores'][30:])
    keep, counts = res['touching_at_zero']
    assert _kept(keep, counts, [0, 4]) == [0, 1, 2, 3]                               # touching boxes give exactly 0.0


# ---- pre_max -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_pre_max_cuts_by_rank(mode):
    for name, c in R.pre_max_cases(mode).items():
        keep, counts = _check(c, name)
        k = c['pre_max']
        for g in (0, 1):
            o0, n = c['off'][g], c['off'][g + 1] - c['off'][g]
            order = o0 + np.lexsort((np.arange(n), -c['scores'][o0:o0 + n]))
            cut = set(order[k:])
            kept = _kept(keep, counts, c['off'], g)
            assert not cut & set(kept), name                       # rows cut by it appear nowhere
            assert kept[0] == order[0] and counts[g] <= k
        if k == 1:
            assert list(counts) == [1, 1]
    full = R.pre_max_cases(mode)
    a, b = _check(full['pre_max_130'])[0], _check(full['pre_max_5000'])[0]
    assert np.array_equal(a, b) and np.array_equal(a, _check(dict(full['pre_max_130'], pre_max=None))[0])


# ---- normal mode ---------------------------------------------------------------------------------------------------------------------
def test_normal_mode_decides_every_pair_like_exact_fractions():
    g = R.grid_crowd(300, 61)
    n = len(g)
    assert np.all(g[:, [0, 1, 3, 4]] * 64 == np.round(g[:, [0, 1, 3, 4]] * 64)) and np.abs(g[:, :2]).max() <= 64
    # one 2-row group per ordered pair: p leads, q is kept iff not v(q, p) > thresh
    c, q, p = R.ordered_pairs_case(g, 0.0)
    off = c['off']
    assert len(q) == n * (n - 1)
    exact = np.array([R.normal_fraction(g[i], g[j]) for i, j in zip(q, p)], dtype=object)
    assert np.mean(exact > 0) > 0.05
    for t in (0.1, 0.25, 0.5, 0.7):
        st, keep, counts = R.host_raw(dict(c, thresh=t))
        assert st == 0
        want = exact > Fraction(t)
        assert 0 < want.sum() < len(want)
        assert np.array_equal(counts == 1, want), (t, np.flatnonzero((counts == 1) != want)[:5])
        assert np.all(keep[0::2] == off[:-1])


def test_normal_mode_ignores_headings_and_position():
    g = R.grid_crowd(300, 61)
    s = R.crowd_scores(300, 9)
    for t in (0.1, 0.25, 0.5, 0.7):
        keep, counts = _check(R.case(g, s, [0, 300], t, 'normal'), t)
        assert 1 < counts[0] < 300
        moved = g.copy()
        moved[:, 0] += 1000.0
        moved[:, 1] += 2048.0
        moved[:, 6] = np.random.default_rng(8).uniform(-3, 3, 300)
        keep2, counts2 = _check(R.case(moved, s, [0, 300], t, 'normal'), t)
        assert np.array_equal(keep, keep2) and np.array_equal(counts, counts2)


# ---- crowds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [129, 512])
@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_crowds_equal_the_reference(n, seed, dtype):
    for t in (0.1, 0.5, 0.7):
        keep, counts = _check(R.crowd_case(n, seed, t, dtype), (n, seed, t))
        if t == 0.5:
            print(f'crowd n {n} seed {seed} {np.dtype(dtype).name}: {counts[0]} kept at 0.5')
            assert 1 < counts[0] < n


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_err_arg_and_groups_above_max_group():
    n = nms.MAX_GROUP + 1
    c = R.case(R.far_boxes(n), np.linspace(1, 0, n), [0, n], 0.5)
    st, keep, counts = R.host_raw(c)
    assert st == 1 and np.all(keep == R.SENTINEL) and np.all(counts == R.SENTINEL)
    with pytest.raises(ValueError, match='off'):
        nms.nms_groups_host(c['boxes'], c['scores'], [0, n], 0.5)
    for mode in MODES:
        c = R.small_group_case(mode)
        keep, counts = _check(c, mode)
        assert counts[1] == -1 and np.all(keep[50:140] == -1) and counts[0] > 1 and counts[2] > 1
    ok = R.case(R.CHAIN, np.array([0.9, 0.8, 0.7]), [0, 3], 0.5)
    b, s, off = ok['boxes'], ok['scores'], np.array([0, 3], np.int32)
    keep, counts = np.zeros(3, np.int32), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(box_dtype=1, boxes=p(b), score_dtype=1, scores=p(s), o=p(off), groups=1, rows=3, max_group=3, mode=0, keep_=p(keep), counts_=p(counts)):
        return lib.vg_boxes_nms_host(box_dtype, boxes, score_dtype, scores, o, groups, rows, max_group, mode, 0.5, 0, keep_, counts_)
    assert call() == 0 and list(keep) == [0, 2, -1]
    for kw in ({'box_dtype': 2}, {'score_dtype': -1}, {'mode': 2}, {'groups': -1}, {'rows': -1}, {'max_group': -1}, {'boxes': None},
               {'scores': None}, {'o': None}, {'keep_': None}, {'counts_': None}):
        assert call(**kw) == 1, kw
    assert call(groups=0, boxes=None) == 0 and call(rows=0, boxes=None) == 0
    assert lib.vg_boxes_nms_work_bytes(0, 10, 1) == 0
    assert lib.vg_boxes_nms_work_bytes(100, 65, 3) >= 100 * 4 + 100 * 2 * 8


# ---- Python --------------------------------------------------------------------------------------------------------------------------
def test_nms_groups_host_call_shape_and_value_errors():
    c = R.seam_case('rotated', np.float32, seed=1)
    wide = np.c_[c['boxes'], np.full((len(c['boxes']), 2), np.nan, np.float32)]                 # only the first 7 columns are read
    keep, counts = nms.nms_groups_host(wide, c['scores'], c['off'], c['thresh'])
    w_keep, w_counts = R.reference(c, sentinel=-1)
    assert keep.dtype == np.int32 and counts.dtype == np.int32 and keep.shape == (len(wide),) and counts.shape == (len(c['off']) - 1,)
    assert np.array_equal(keep, w_keep) and np.array_equal(counts, w_counts)
    k2, c2 = nms.nms_groups_host(wide, c['scores'], c['off'], c['thresh'], mode='rotated', pre_maxsize=10 ** 6)
    assert np.array_equal(k2, keep) and np.array_equal(c2, counts)
    b, s = c['boxes'], c['scores']
    for kw, name in (({'mode': 'bev'}, 'mode'), ({'off': [0, 5, 3]}, 'off'), ({'off': [0, len(b) + 1]}, 'off'), ({'off': [-1, 4]}, 'off'),
                     ({'off': [[0, 1]]}, 'off'), ({'pre_maxsize': 0}, 'pre_maxsize'), ({'boxes': b[:, :6]}, 'boxes'), ({'scores': s[:-1]}, 'scores')):
        args = dict(boxes=b, scores=s, off=[0, 5], thresh=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            nms.nms_groups_host(**args)


def test_device_wrappers_refuse_what_they_cannot_take():
    import torch
    b, s = torch.zeros(4, 7), torch.zeros(4)
    for fn in (nms.nms_gpu, nms.nms_normal_gpu):
        with pytest.raises(ValueError, match='CUDA'):
            fn(b, s, 0.5)
    with pytest.raises(ValueError, match='CUDA'):
        nms.nms_groups(b, s, [0, 4], 0.5)
    import inspect
    for fn in (nms.nms_gpu, nms.nms_normal_gpu):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:4] == ['boxes', 'scores', 'thresh', 'pre_maxsize'] and sig.parameters['pre_maxsize'].default is None
        assert any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())
    assert list(inspect.signature(nms.nms_groups).parameters)[:7] == ['boxes', 'scores', 'off', 'thresh', 'mode', 'pre_maxsize', 'stream']


def test_label_proposals_checks_its_nms_arguments_before_any_device_work():
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pipe = PseudoLabelPipeline.__new__(PseudoLabelPipeline)        # the checks run before anything of the instance is touched
    props, pts, pose = np.zeros((3, 7)), np.zeros((10, 4), np.float32), np.eye(4)
    with pytest.raises(ValueError, match='scores'):
        pipe.label_proposals(pts, pose, pose, props, nms={'thresh': 0.5})
    with pytest.raises(ValueError, match='scores'):
        pipe.label_proposals(pts, pose, pose, props, scores=np.zeros(2), nms={'thresh': 0.5})
    with pytest.raises(ValueError, match='nms'):
        pipe.label_proposals(pts, pose, pose, props, scores=np.zeros(3), nms={'mode': 'rotated'})
    with pytest.raises(ValueError, match='nms'):
        pipe.label_proposals(pts, pose, pose, props, scores=np.zeros(3), nms={'thresh': 0.5, 'top': 3})
    with pytest.raises(ValueError, match='mode'):
        pipe.label_proposals(pts, pose, pose, props, scores=np.zeros(3), nms={'thresh': 0.5, 'mode': 'bev'})
