"""All seven cluster filters of the reference with its and / or / required logic (csrc/segment.hip k_cluster_filter_ex,
PseudoLabelPipeline.filter).  The reference's own verdicts are in tests/golden/filters_golden.npz (tests/golden/make_filters.py);
tests/filters_ref.py restates the filters in numpy / float64.

Bounds.  Number of points, height, plane distance, aspect ratio and ephemeral score are compared with the reference on EVERY
cluster, the percentile bit for bit with the restatement.  The kernel's float64 hull area is compared with the correctly rounded
exact area under filters_ref.area_bound_f64 (float64 rounding of H terms).  Area / volume verdicts are compared with the
reference's on every cluster whose float64 value is farther from each threshold than the reference's own float32 shoelace bound
B = (H+2)/2 * 2^-24 * sum(|x_i y_j| + |x_j y_i|) (x height for the volume); at most 5 % of the clusters may be left out per
threshold set, and at least 20 clusters must be compared on each side of each threshold.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import filters_ref as fr
from conftest import ROOT

N, H, R, V, A, P, E = fr.FILTER_NAMES
ALL_SEVEN = [dict(name=N, args=dict(logic='and', required=True, min_points=10)),
             dict(name=H, args=dict(logic='and', required=True, min_height=0.3, max_height=6)),
             dict(name=R, args=dict(logic='and', min_aspect_ratio=1.0, max_aspect_ratio=5.0)),
             dict(name=V, args=dict(logic='and', min_volume=0.5)),
             dict(name=A, args=dict(logic='and', min_area=0.35)),
             dict(name=P, args=dict(logic='and', required=True, max_min_height=1.0, min_max_height=0.5)),
             dict(name='filter_by_density', args=dict(min_density=0.1, max_density=10)),
             dict(name=E, args=dict(logic='or', percentile=20, min_percentile_pp_score=0.7))]


@pytest.fixture(scope='module')
def fx(golden_dir):
    return fr.load_fixture(os.path.join(golden_dir, 'filters_golden.npz'))


@pytest.fixture(scope='module')
def fx_stats(fx):
    seg = fx['seg']
    T = fx['meta']['thresholds'][0]
    return [fr.cluster_stats(fx['points'][seg[c]:seg[c + 1]], None, fx['plane'], T) for c in range(len(seg) - 1)]


def _ccfg(filters=ALL_SEVEN, active=None):
    return dict(filters=filters, filters_active=[f['name'] for f in filters] if active is None else active)


def _set_q(stats, fx, T):
    seg = fx['seg']
    for c, st in enumerate(stats):
        st['q'] = fr.percentile(fx['scores'][seg[c]:seg[c + 1]], T[E]['percentile'])


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_all_seven_filters_with_mixed_logic_parse():
    from vilgod_amd.pipeline import PseudoLabelPipeline
    f = PseudoLabelPipeline._parse_filters(_ccfg())
    assert f['active'] == [N, H, R, V, A, P, E]                      # filter_by_density: not defined by cluster_utils, skipped
    assert f['logic'][N] == ('and', True) and f['logic'][V] == ('and', False) and f['logic'][E] == ('or', False)
    assert f['entry'] == 'vg_cluster_filter_ex' and f['needs_entropy'] and f['use_plane']
    p = f['params']
    assert list(p.active) == [1] * 7 and list(p.logic) == [0, 0, 1, 1, 1, 0, 2]
    assert (p.min_points, p.max_points, p.min_area, p.has_max_area, p.percentile) == (10, 999999, 0.35, 0, 20.0)
    f = PseudoLabelPipeline._parse_filters(_ccfg([dict(name=A, args=dict(logic='or', min_area=1.0, max_area=9.0)),
                                                  dict(name=V, args=dict(logic='and', min_volume=1.0, max_volume=None))]))
    assert (f['params'].has_max_area, f['params'].max_area, f['params'].has_max_volume) == (1, 9.0, 0)


def test_missing_logic_raises_value_error():
    from vilgod_amd.pipeline import PseudoLabelPipeline
    shipped_entry = [dict(name=R, args=dict(min_aspect_ratio=1.0, max_aspect_ratio=5.0))]      # waymo.yaml:32-35 has no `logic`
    with pytest.raises(ValueError, match='filter_by_aspect_ratio'):
        PseudoLabelPipeline._parse_filters(_ccfg(shipped_entry))
    with pytest.raises(ValueError):
        PseudoLabelPipeline._parse_filters(_ccfg([dict(name=A, args=dict(logic='xor', min_area=1.0))]))
    PseudoLabelPipeline._parse_filters(_ccfg(shipped_entry, active=[]))                        # inactive: never looked at


def test_ephemeral_filter_without_entropy_stage_raises():
    from vilgod_amd.pipeline import PseudoLabelPipeline
    f = PseudoLabelPipeline._parse_filters(_ccfg())
    with pytest.raises(ValueError, match='calculate_entropy_scores'):
        PseudoLabelPipeline.check_filter_stages(f, ['mask_ground_points', 'spatial_clustering', 'filter_detections'])
    PseudoLabelPipeline.check_filter_stages(f, ['mask_ground_points', 'calculate_entropy_scores', 'spatial_clustering', 'filter_detections'])
    g = PseudoLabelPipeline._parse_filters(_ccfg(active=[N, A]))
    PseudoLabelPipeline.check_filter_stages(g, ['mask_ground_points', 'spatial_clustering', 'filter_detections'])


def test_density_is_skipped_and_shipped_config_keeps_the_old_entry():
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    f = PseudoLabelPipeline._parse_filters(default_preprocessor_cfg()['clustering'])
    assert f['entry'] == 'vg_cluster_filter' and not f['needs_entropy'] and sorted(f['active']) == sorted([N, H, P])
    assert (f['min_points'], f['min_height'], f['max_height'], f['max_min_height'], f['min_max_height']) == (10, 0.3, 6, 1.0, 0.5)
    f = PseudoLabelPipeline._parse_filters(_ccfg(active=[N, H, P, 'filter_by_density']))
    assert f['entry'] == 'vg_cluster_filter' and 'filter_by_density' not in f['active']
    # the same three filters with another combination class are no longer the shipped set
    relaxed = [dict(f, args=dict(f['args'], required=False)) if f['name'] == H else f for f in ALL_SEVEN]
    assert PseudoLabelPipeline._parse_filters(_ccfg(relaxed, active=[N, H, P]))['entry'] == 'vg_cluster_filter_ex'


def test_new_entry_is_exported_and_declared():
    from vilgod_amd import _lib
    protos = _lib.parse_header()
    assert 'vg_cluster_filter_ex' in protos and len(protos['vg_cluster_filter_ex'][1]) == 12
    assert hasattr(_lib.lib, 'vg_cluster_filter_ex') and hasattr(_lib.lib, 'vg_filter_default_params')
    p = _lib.FilterParams()
    assert list(p.active) == [0] * 7 and p.max_points == 999999 and p.has_max_area == 0
    assert ctypes.sizeof(p) == 14 * 4 + 4 * 4 + 12 * 8


def test_new_kernel_uses_no_scratch():
    from vilgod_amd import build
    assert build.check_scratch('segment.hip', 'k_cluster_filter_ex') == []
    assert build.check_isa(sources=['segment.hip']) == []


def test_restatement_reproduces_reference(fx, fx_stats):
    C = len(fx['seg']) - 1
    assert C >= 200
    for ti, T in enumerate(fx['meta']['thresholds']):
        _set_q(fx_stats, fx, T)
        mine = [fr.verdicts(st, T) for st in fx_stats]
        for name in (N, H, R, P, E):
            assert [m[name] for m in mine] == list(fx[f'ref_{ti}_{name}']), (ti, name)
        for name, key in ((A, 'area'), (V, 'volume')):
            cmp = _comparable(fx_stats, T, name, key)
            assert [mine[c][name] for c in np.flatnonzero(cmp)] == list(fx[f'ref_{ti}_{name}'][cmp]), (ti, name)


def _comparable(stats, T, name, key):
    """clusters farther from every threshold of `name` than the reference's float32 bound; asserts the coverage conditions"""
    thr = [T[name]['min_' + key]] + ([T[name]['max_' + key]] if T[name].get('max_' + key) is not None else [])
    scale = (lambda st: 1.0) if key == 'area' else (lambda st: float(st['height']))
    val = np.array([st[key] for st in stats])
    band = np.array([fr.band_f32(st['n_hull'], st['S']) * scale(st) for st in stats])
    cmp = np.all([np.abs(val - t) > band for t in thr], axis=0)
    assert (~cmp).mean() <= 0.05
    for t in thr:
        assert ((val < t) & cmp).sum() >= 20 and ((val > t) & cmp).sum() >= 20
    return cmp


def test_combination_truth_table(fx):
    """(all(and) or any(or)) and all(required) against Detection.filter, for every logic assignment of the fixture, from the
    reference's own per-filter verdicts"""
    seen = set()
    for ti in range(len(fx['meta']['thresholds'])):
        for li, L in enumerate(fx['meta']['logic']):
            logic = {k: tuple(v) for k, v in L.items()}
            for c in range(len(fx['seg']) - 1):
                v = {k: bool(fx[f'ref_{ti}_{k}'][c]) for k in logic}
                assert fr.combine(v, logic) == bool(fx[f'comb_{ti}'][li, c]), (ti, li, c)
                a = [v[k] for k, (lg, rq) in logic.items() if lg == 'and' and not rq]
                o = [v[k] for k, (lg, rq) in logic.items() if lg == 'or']
                r = [v[k] for k, (lg, rq) in logic.items() if lg == 'and' and rq]
                seen.add((bool(a), all(a), bool(o), any(o), bool(r), all(r)))
    # every branch: empty and non-empty lists of each class, each both satisfied and not
    for i in range(0, 6, 2):
        assert {(s[i], s[i + 1]) for s in seen} == {(False, True if i != 2 else False), (True, True), (True, False)}


# ------------------------------------------------------------------------------------------------------------------- GPU
def _params(T, logic):
    from vilgod_amd._lib import FilterParams, FILTER_NAMES
    p = FilterParams()
    for name, (lg, req) in logic.items():
        k = FILTER_NAMES.index(name)
        p.active[k] = 1
        p.logic[k] = 2 if lg == 'or' else (0 if req else 1)
    p.min_points, p.max_points = T[N].get('min_points', 0), T[N].get('max_points', 999999)
    p.min_height, p.max_height = T[H]['min_height'], T[H]['max_height']
    p.min_aspect_ratio, p.max_aspect_ratio = T[R]['min_aspect_ratio'], T[R]['max_aspect_ratio']
    p.min_volume, p.min_area = T[V]['min_volume'], T[A]['min_area']
    if T[V].get('max_volume') is not None:
        p.has_max_volume, p.max_volume = 1, T[V]['max_volume']
    if T[A].get('max_area') is not None:
        p.has_max_area, p.max_area = 1, T[A]['max_area']
    p.max_min_height, p.min_max_height = T[P]['max_min_height'], T[P]['min_max_height']
    p.percentile, p.min_percentile_pp_score = T[E]['percentile'], T[E]['min_percentile_pp_score']
    return p


GUARD = 0xA5


def _run_ex(cuda, points, seg, plane, scores, p, stride=4, shuffle_seed=None):
    """vg_cluster_filter_ex through the C ABI on packed clusters -> stats [C,16] f64, verdict [C,7] bool, valid [C] bool.
    The points sit in rows of `stride` floats and are addressed through a permuted index list; d_verdict / d_valid carry guard
    bytes on both sides."""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    n, C = len(points), len(seg) - 1
    rng = np.random.default_rng(0 if shuffle_seed is None else shuffle_seed)
    perm = rng.permutation(n)                                  # row of point i in the device array
    rows = np.zeros((n, stride), np.float32)
    rows[perm, :3] = points
    rows[:, 3:] = 7.0
    sc = np.zeros(n, np.float32)
    if scores is not None:
        sc[perm] = scores
    d_pts = torch.from_numpy(rows).to(cuda)
    d_sc = torch.from_numpy(sc).to(cuda) if scores is not None else None
    d_idx = torch.from_numpy(perm.astype(np.int32)).to(cuda)
    d_seg = torch.from_numpy(np.asarray(seg, np.int32)).to(cuda)
    d_plane = torch.from_numpy(np.asarray(plane, np.float64)).to(cuda)
    stats = torch.full((C, 16), -777.0, dtype=torch.float64, device=cuda)
    verdict = torch.full((C * 7 + 128,), GUARD, dtype=torch.uint8, device=cuda)
    valid = torch.full((C + 128,), GUARD, dtype=torch.uint8, device=cuda)
    check(lib.vg_cluster_filter_ex(ptr(d_pts), stride, ptr(d_idx), ptr(d_seg), C, ptr(d_plane), ptr(d_sc), ctypes.byref(p), ptr(stats),
                                   ctypes.c_void_p(verdict.data_ptr() + 64), ctypes.c_void_p(valid.data_ptr() + 64), stream_ptr()),
          'vg_cluster_filter_ex')
    torch.cuda.synchronize()
    verdict, valid = verdict.cpu().numpy(), valid.cpu().numpy()
    assert (verdict[:64] == GUARD).all() and (verdict[64 + C * 7:] == GUARD).all(), 'guard bytes around d_verdict'
    assert (valid[:64] == GUARD).all() and (valid[64 + C:] == GUARD).all(), 'guard bytes around d_valid'
    assert set(np.unique(verdict[64:64 + C * 7])) <= {0, 1} and set(np.unique(valid[64:64 + C])) <= {0, 1}
    return stats.cpu().numpy(), verdict[64:64 + C * 7].reshape(C, 7).astype(bool), valid[64:64 + C].astype(bool), (d_pts, d_idx, d_seg, d_plane)


@pytest.mark.gpu
def test_kernel_verdicts_equal_reference_on_every_cluster(cuda, fx, fx_stats):
    from vilgod_amd._lib import FILTER_NAMES
    assert tuple(FILTER_NAMES) == fr.FILTER_NAMES
    seg, C = fx['seg'], len(fx['seg']) - 1
    all_and = {k: ('and', False) for k in fr.FILTER_NAMES}
    for ti, T in enumerate(fx['meta']['thresholds']):
        stats, verdict, valid, _ = _run_ex(cuda, fx['points'], seg, fx['plane'], fx['scores'], _params(T, all_and))
        _set_q(fx_stats, fx, T)
        for name in (N, H, R, P, E):
            k = fr.FILTER_NAMES.index(name)
            bad = np.flatnonzero(verdict[:, k] != fx[f'ref_{ti}_{name}'])
            print(f'set {ti} {name}: {len(bad)} of {C} verdicts differ from the reference')
            assert len(bad) == 0, (ti, name, bad[:10])
        q = np.array([st['q'] for st in fx_stats])
        print(f'set {ti}: percentile values differing from the restatement: {(stats[:, 13].view(np.int64) != q.view(np.int64)).sum()}')
        assert np.array_equal(stats[:, 13].view(np.int64), q.view(np.int64))
        # extents and ratio: single correctly rounded float32 operations
        for col, key in ((5, 'height'), (6, 'size_x'), (7, 'size_y'), (8, 'ratio')):
            want = np.array([st[key] for st in fx_stats], np.float32)
            assert np.array_equal(stats[:, col].astype(np.float32).view(np.int32), want.view(np.int32)), key
        # area: float64 rounding of H terms
        want = np.array([st['area'] for st in fx_stats])
        bound = np.array([fr.area_bound_f64(st['n_hull'], st['S']) for st in fx_stats])
        err = np.abs(stats[:, 9] - want)
        print(f'set {ti}: area error / bound max {np.max(err / bound):.3f}; hull vertices up to {int(stats[:, 11].max())}')
        assert np.all(err <= bound)
        assert np.array_equal(stats[:, 11].astype(int), [st['n_hull'] for st in fx_stats])
        assert not stats[:, 12].any()
        assert np.all(np.abs(stats[:, 14] - [st['S'] for st in fx_stats]) <= 1e-12 * stats[:, 14])
        assert np.array_equal(stats[:, 10], stats[:, 9] * stats[:, 5])
        for name, key in ((A, 'area'), (V, 'volume')):
            k = fr.FILTER_NAMES.index(name)
            cmp = _comparable(fx_stats, T, name, key)
            bad = np.flatnonzero((verdict[:, k] != fx[f'ref_{ti}_{name}']) & cmp)
            print(f'set {ti} {name}: {int((~cmp).sum())} of {C} inside the band, {len(bad)} compared verdicts differ')
            assert len(bad) == 0, (ti, name, bad[:10])
        assert np.array_equal(valid, verdict.all(axis=1))


@pytest.mark.gpu
def test_kernel_combination_equals_detection_filter(cuda, fx, fx_stats):
    seg = fx['seg']
    for ti, T in enumerate(fx['meta']['thresholds']):
        cmp = _comparable(fx_stats, T, A, 'area') & _comparable(fx_stats, T, V, 'volume')
        for li, L in enumerate(fx['meta']['logic']):
            logic = {k: tuple(v) for k, v in L.items()}
            stats, verdict, valid, _ = _run_ex(cuda, fx['points'], seg, fx['plane'], fx['scores'], _params(T, logic), stride=3, shuffle_seed=li)
            inactive = [k for k, name in enumerate(fr.FILTER_NAMES) if name not in logic]
            assert not verdict[:, inactive].any()
            assert np.array_equal(valid[cmp], fx[f'comb_{ti}'][li][cmp]), (ti, li)
            want = [fr.combine({k: bool(verdict[c, fr.FILTER_NAMES.index(k)]) for k in logic}, logic) for c in range(len(seg) - 1)]
            assert np.array_equal(valid, want), (ti, li)


@pytest.mark.gpu
def test_shipped_filters_through_either_entry_give_the_same_bits(cuda, fx):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    seg, C = fx['seg'], len(fx['seg']) - 1
    for T in fx['meta']['thresholds']:
        logic = {N: ('and', True), H: ('and', True), P: ('and', True)}
        stats, verdict, valid, (d_pts, d_idx, d_seg, d_plane) = _run_ex(cuda, fx['points'], seg, fx['plane'], None, _params(T, logic))
        stats6 = torch.empty((C, 6), dtype=torch.float32, device=cuda)
        valid0 = torch.empty(C, dtype=torch.uint8, device=cuda)
        check(lib.vg_cluster_filter(ptr(d_pts), 4, ptr(d_idx), ptr(d_seg), C, ptr(d_plane), T[N].get('min_points', 0),
                                    T[N].get('max_points', 999999), T[P]['max_min_height'], T[P]['min_max_height'], T[H]['min_height'],
                                    T[H]['max_height'], ptr(stats6), ptr(valid0), stream_ptr()), 'vg_cluster_filter')
        assert np.array_equal(valid0.cpu().numpy().astype(bool), valid)
        assert np.array_equal(stats6.cpu().numpy().view(np.int32), stats[:, :6].astype(np.float32).view(np.int32))


def _one(cuda, pts, scores=None, logic=None, T=None, plane=(0.0, 0.0, 1.0, 1.7)):
    T = T or dict({N: {}, H: dict(min_height=-1.0, max_height=100.0), R: dict(min_aspect_ratio=1.0, max_aspect_ratio=5.0),
                   V: dict(min_volume=0.0), A: dict(min_area=0.0), P: dict(max_min_height=100.0, min_max_height=-100.0),
                   E: dict(percentile=20, min_percentile_pp_score=0.7)})
    logic = logic or {k: ('and', False) for k in fr.FILTER_NAMES if k != E or scores is not None}
    pts = np.asarray(pts, np.float32)
    stats, verdict, valid, _ = _run_ex(cuda, pts, [0, len(pts)], plane, scores, _params(T, logic))
    return stats[0], dict(zip(fr.FILTER_NAMES, verdict[0])), valid[0]


@pytest.mark.gpu
def test_stated_behaviour_degenerate_clusters(cuda):
    """collinear / identical points (the reference dies in qhull): area 0, verdict `0 >= min_area`, degenerate flag; fewer than 3
    points: false; zero xy extents: x/0 = inf, 0/0 = nan, comparisons with nan false"""
    t = np.linspace(0, 1, 30)
    z = np.linspace(-1, 0.5, 30)
    for name, xy in (('collinear_x', np.stack([t * 5 + 3, np.full(30, 2.5)], 1)), ('collinear_diag', np.stack([t * 3 + 7, t * 3 + 7], 1)),
                     ('identical', np.full((30, 2), 4.25))):
        pts = np.concatenate([xy, z[:, None]], 1)
        st, v, _ = _one(cuda, pts)
        assert st[9] == 0.0 and st[10] == 0.0 and int(st[12]) == 1, name
        assert v[A] and v[V], name                                      # 0 >= min_area = 0
        T1 = dict({N: {}, H: dict(min_height=-1.0, max_height=100.0), R: dict(min_aspect_ratio=1.0, max_aspect_ratio=5.0),
                   V: dict(min_volume=0.5), A: dict(min_area=0.35), P: dict(max_min_height=100.0, min_max_height=-100.0),
                   E: dict(percentile=20, min_percentile_pp_score=0.7)})
        st, v, _ = _one(cuda, pts, T=T1)
        assert not v[A] and not v[V] and int(st[12]) == 1, name
    # zero y extent: ratio = 5/0 = inf -> max fails; identical: 0/0 = nan -> max_valid false
    st, v, _ = _one(cuda, np.concatenate([np.stack([t * 5 + 3, np.full(30, 2.5)], 1), z[:, None]], 1))
    assert np.isinf(st[8]) and not v[R]
    st, v, _ = _one(cuda, np.concatenate([np.full((30, 2), 4.25), z[:, None]], 1))
    assert np.isnan(st[8]) and not v[R]
    # two points: area / volume false whatever the thresholds, no flag
    st, v, _ = _one(cuda, [[1.0, 2.0, 0.0], [2.0, 3.5, 1.0]])
    assert not v[A] and not v[V] and int(st[12]) == 0 and st[0] == 2 and v[N] and v[R]
    # three points: a proper triangle
    st, v, _ = _one(cuda, [[10.0, 20.0, 0.0], [12.0, 20.0, 1.0], [10.0, 23.0, 0.5]])
    assert st[9] == 3.0 and st[10] == 3.0 and st[11] == 3 and v[A] and v[V]


@pytest.mark.gpu
def test_no_clusters_and_argument_checks(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, FilterParams
    p = FilterParams()
    assert lib.vg_cluster_filter_ex(None, 4, None, None, 0, None, None, ctypes.byref(p), None, None, None, stream_ptr()) == 0
    p.active[6], p.logic[6] = 1, 2
    d = torch.zeros(16, dtype=torch.float32, device=cuda)
    di = torch.zeros(4, dtype=torch.int32, device=cuda)
    assert lib.vg_cluster_filter_ex(ptr(d), 4, ptr(di), ptr(di), 1, ptr(d), None, ctypes.byref(p), ptr(d), ptr(d), ptr(d), stream_ptr()) == 1
    p.active[6], p.active[0], p.logic[0] = 0, 1, 5
    assert lib.vg_cluster_filter_ex(ptr(d), 4, ptr(di), ptr(di), 1, ptr(d), None, ctypes.byref(p), ptr(d), ptr(d), ptr(d), stream_ptr()) == 1


def _circle(n, r=20.0, centre=(30.0, -12.0)):
    phi = 2 * np.pi * np.arange(n) / n
    xy = np.stack([centre[0] + r * np.cos(phi), centre[1] + r * np.sin(phi)], 1)
    return np.concatenate([xy, np.linspace(-1.5, 0.5, n)[:, None]], 1).astype(np.float32)


@pytest.mark.gpu
def test_hull_beyond_capacity_is_flagged_and_the_pipeline_uses_the_host_area(cuda):
    import torch
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg, host_hull_area
    pts = _circle(2000)
    v_ref = fr.hull_ccw(pts[:, :2])
    assert len(v_ref) > fr.HULL_CAPACITY
    st, v, valid = _one(cuda, pts)
    assert int(st[12]) == 2 and not v[A] and not v[V] and not valid            # flagged, never a silent verdict
    # a 1 000-vertex circle fits
    small = _circle(1000)
    st, v, _ = _one(cuda, small)
    want, S = fr.shoelace(small[:, :2], fr.hull_ccw(small[:, :2]))
    assert int(st[12]) == 0 and st[11] == 1000 and abs(st[9] - want) <= fr.area_bound_f64(1000, S)
    cfg = default_preprocessor_cfg()
    cfg['clustering']['filters'] = [dict(name=A, args=dict(logic='and', required=True, min_area=1000.0, max_area=1300.0)),
                                    dict(name=V, args=dict(logic='and', min_volume=2400.0))]
    cfg['clustering']['filters_active'] = [A, V]
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=16_000, clip_model_path='/nonexistent')
    both = np.concatenate([pts, small])
    d_X = torch.from_numpy(both).to(cuda)
    d_index = torch.arange(len(both), dtype=torch.int32, device=cuda)
    d_seg = torch.tensor([0, 2000, 3000], dtype=torch.int32, device=cuda)
    valid, stats6 = pipe.filter(d_X, d_index, d_seg, np.array([0.0, 0.0, 1.0, 1.7]))
    area, nh = host_hull_area(pts[:, :2])
    exact, S = fr.shoelace(pts[:, :2], v_ref)
    assert abs(area - exact) <= fr.area_bound_f64(len(v_ref), S) and nh == len(v_ref)
    full = pipe.last_filter_stats.cpu().numpy()
    assert full[0, 9] == area and full[0, 10] == area * full[0, 5] and full[0, 11] == nh
    assert 1000.0 <= area <= 1300.0 and area * 2.0 >= 2400.0                   # pi * 20^2 = 1256.6, height 2
    assert list(pipe.last_filter_dict[A]) == [True, True] and list(pipe.last_filter_dict[V]) == [True, True]
    assert list(valid.cpu().numpy()) == [1, 1] and stats6.shape == (2, 6)


@pytest.mark.gpu
def test_one_50000_point_cluster(cuda, fx, fx_stats):
    c = int(np.argmax(np.diff(fx['seg'])))
    lo, hi = fx['seg'][c], fx['seg'][c + 1]
    assert hi - lo == 50_000
    T = fx['meta']['thresholds'][0]
    st, v, _ = _one(cuda, fx['points'][lo:hi], scores=fx['scores'][lo:hi], T=T, plane=fx['plane'])
    want = fx_stats[c]
    assert st[0] == 50_000 and st[11] == want['n_hull']
    assert abs(st[9] - want['area']) <= fr.area_bound_f64(want['n_hull'], want['S'])
    assert np.float64(st[13]).view(np.int64) == np.float64(fr.percentile(fx['scores'][lo:hi], 20)).view(np.int64)
    for name in (N, H, R, P, E):
        assert v[name] == fx[f'ref_0_{name}'][c], name


def _kitti(golden_dir, i):
    return np.fromfile(f'{golden_dir}/kitti_00000{i}.bin', dtype=np.float32).reshape(-1, 4)


@pytest.mark.gpu
def test_pipeline_with_all_filters_matches_the_restatement(cuda, golden_dir):
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    from vilgod_amd.entropy import full_scores
    cfg = default_preprocessor_cfg()
    cfg['clustering']['filters'] = ALL_SEVEN
    cfg['clustering']['filters_active'] = [f['name'] for f in ALL_SEVEN]
    frames = [_kitti(golden_dir, i) for i in range(4)]
    poses = [np.eye(4) for _ in frames]
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=140_000, clip_model_path='/nonexistent')
    assert pipe._filters['entry'] == 'vg_cluster_filter_ex'
    got = pipe.process_sequence(frames, poses, poses[0], entropy_args=dict(n_neighbouring_frames=3, skip_frames=0), n_frames=2, seed=0)
    T = {f['name']: f['args'] for f in ALL_SEVEN}
    logic = {f['name']: (f['args']['logic'], bool(f['args'].get('required', False))) for f in ALL_SEVEN if f['name'] in fr.FILTER_NAMES}
    n_clusters = n_or = n_band = 0
    for (fs, _), pts in zip(got, frames):
        gm = np.zeros(len(pts), bool)
        gm[fs.ground_point_indices] = True
        X = pts[~gm][:, :3]                                               # identity poses: points_ref_wo_ground
        ent = full_scores(len(X), fs.entropy_scores, fs.entropy_indices)
        assert sorted(fs.filter_dict) == sorted(logic) and fs.filtered
        for c in range(fs.n_detections):
            idx = fs.cluster_index(c)
            st = fr.cluster_stats(X[idx], ent[idx], fs.ground_plane_model_ref, T)
            v = fr.verdicts(st, T)
            near = any(abs(st[k] - t) <= fr.area_bound_f64(st['n_hull'], st['S']) * s for k, t, s in
                       (('area', T[A]['min_area'], 1.0), ('volume', T[V]['min_volume'], float(st['height']))))
            n_band += near
            if near:
                continue                                                  # within float64 rounding of a threshold
            for name in logic:
                assert bool(fs.filter_dict[name][c]) == v[name], (fs.fnr, c, name)
            assert bool(fs.valid[c]) == fr.combine(v, logic), (fs.fnr, c)
            n_clusters += 1
            n_or += v[E] and not all(v[k] for k in (R, V, A))
    print(f'{n_clusters} clusters compared, {n_band} within float64 rounding of a threshold, {n_or} kept by the `or` filter alone')
    assert n_clusters >= 100 and n_band <= 2


@pytest.mark.gpu
def test_pipeline_with_the_shipped_config_is_unchanged(cuda, golden_dir):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    pipe = PseudoLabelPipeline(default_preprocessor_cfg(), device=cuda, vit_dtype='f16', max_points=140_000, clip_model_path='/nonexistent')
    assert pipe._filters['entry'] == 'vg_cluster_filter'
    pts = _kitti(golden_dir, 0)
    fs, _ = pipe.process_frame(pts, np.eye(4), np.eye(4), fnr=0)
    assert fs.filter_dict == {} and pipe.last_filter_dict is None and fs.n_detections > 20
    gm = np.zeros(len(pts), bool)
    gm[fs.ground_point_indices] = True
    d_X = torch.from_numpy(np.ascontiguousarray(pts[~gm])).to(cuda)
    d_index, d_seg = torch.from_numpy(fs.index).to(cuda), torch.from_numpy(fs.seg_off).to(cuda)
    C = fs.n_detections
    stats, valid = torch.empty((C, 6), dtype=torch.float32, device=cuda), torch.empty(C, dtype=torch.uint8, device=cuda)
    d_plane = torch.from_numpy(np.asarray(fs.ground_plane_model_ref, np.float64)).to(cuda)
    check(lib.vg_cluster_filter(ptr(d_X), 4, ptr(d_index), ptr(d_seg), C, ptr(d_plane), 10, 999999, 1.0, 0.5, 0.3, 6.0, ptr(stats), ptr(valid),
                                stream_ptr()), 'vg_cluster_filter')
    assert np.array_equal(valid.cpu().numpy().astype(bool), fs.valid)
    v2, s2 = pipe.filter(d_X, d_index, d_seg, fs.ground_plane_model_ref)
    assert torch.equal(v2, valid) and torch.equal(s2, stats)


@pytest.mark.gpu
def test_ephemeral_filter_without_scores_raises_at_the_first_frame(cuda):
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['clustering']['filters'] = ALL_SEVEN
    cfg['clustering']['filters_active'] = [N, E]
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=16_000, clip_model_path='/nonexistent')
    poses = synthetic.make_poses(2)
    with pytest.raises(ValueError, match='calculate_entropy_scores'):
        pipe.process_frame(synthetic.make_frame(5, 12_000, n_objects=8), poses[1], poses[0], fnr=1)


@pytest.mark.gpu
def test_cli_run_with_a_filters_active_override(cuda, tmp_path):
    import pickle
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    root = str(tmp_path / 'd')
    active = [N, P, H, V, A, E]
    preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', 'preprocessor.clustering.filters_active=[' + ','.join(active) + ']',
                          'dataset.SYNTHETIC.frames_per_sequence=6', 'dataset.SYNTHETIC.points_per_frame=20000',
                          'dataset.SYNTHETIC.objects_per_frame=10', 'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0',
                          'device.max_points=24000', 'paths.clip_model=/nonexistent'])
    with open(f'{root}/preprocessed_data/vilgod_mi355x_seq/synthetic_train_0000.pkl', 'rb') as f:
        state = pickle.load(f)
    dets = [d for frame in state for d in frame['_detections']]
    assert len(dets) > 20 and any(d['valid'] for d in dets) and not all(d['valid'] for d in dets)
    assert any('_bounding_box' in d for d in dets)
