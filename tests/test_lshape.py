"""L-shape box fits of fit_bounding_boxes_simple: closeness_rectangle and variance_rectangle (csrc/lshape.hip, vg_cluster_lshape).

CPU: the restatement (tests/lshape_ref.py) against the reference's own outputs (tests/golden/lshape_golden.npz, made by
     tests/golden/make_lshape.py), the entry point's argument checks, the stage's method handling and the angle tables.
GPU: the kernel against the golden and the restatement (64 golden clusters, the real clusters of detect_golden.pkl, 2 000 random
     clusters), repeatability, and the detector end to end (static and still tracks, moving tracks, both box modes).
"""
import ctypes
import os
import pickle
import sys
import types

import numpy as np
import pytest

import lshape_ref as lr
from conftest import ROOT

VG_OK, VG_ERR_ARG = 0, 1
METHODS = [('closeness_rectangle', 'closeness', 1e-6), ('variance_rectangle', 'variance', 1e-9)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(f'{golden_dir}/lshape_golden.npz'))


def _clusters(g):
    P, seg = g['points'], g['seg']
    return [P[seg[c]:seg[c + 1]] for c in range(len(seg) - 1)]


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('name,key,_tol', METHODS)
def test_restatement_reproduces_reference(golden, name, key, _tol):
    """Plain-numpy evaluation (what the golden recorded): the same criterion of every angle, index, corners and box."""
    for c, p in enumerate(_clusters(golden)):
        k, corners, rz, crit = lr.fit(p[:, :2], name, numba=False)
        assert np.array_equal(crit, golden[f'{key}_crit'][c]), (c, golden['kind'][c])
        assert k == golden[f'{key}_index'][c]
        assert np.array_equal(corners, golden[f'{key}_corners'][c])
        assert rz == golden[f'{key}_angle'][c]
        assert np.array_equal(lr.box(corners, rz, p[:, 2]), golden[f'{key}_box'][c])


@pytest.mark.parametrize('name,key,tol', METHODS)
def test_float64_accumulation_picks_the_reference_angle(golden, name, key, tol):
    """numba's float64 sum of 1 / beta (and the all-angles form) choose the golden's index except at genuine near-ties."""
    ties = 0
    for c, p in enumerate(_clusters(golden)):
        crit = lr.criteria(p[:, :2], name)
        assert np.allclose(lr.criteria_fast(p[:, :2], name), crit, rtol=1e-9, atol=1e-15)
        k, want = int(np.argmax(crit)), golden[f'{key}_index'][c]
        if k != want:
            assert lr.near_tie(golden[f'{key}_crit'][c], k, want, tol), (c, golden['kind'][c])
            ties += 1
    print(f'{name}: {ties} near-ties between float64 and the recorded float32 criteria')
    assert ties <= 1


def test_golden_covers_the_cases(golden):
    kinds = set(golden['kind'].tolist())
    assert {'car', 'pedestrian', 'wall', 'axis_rect', 'rect_45', 'one_point', 'two_points', 'collinear_x', 'duplicated',
            'wall_20k'} <= kinds
    assert len(golden['seg']) - 1 == 64 and np.diff(golden['seg']).max() == 20000
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'lshape_golden.npz')) < 800_000


def test_lshape_entry_point_checks_arguments():
    """vg_cluster_lshape is exported and refuses bad arguments before any device work (no GPU needed)."""
    from vilgod_amd._lib import lib
    fake = ctypes.c_void_p(16)                                  # never dereferenced: every call below returns before device work

    def call(n_clusters=1, criterion=0, n_angles=46, delta_zero=1e-2, ptrs=True, stride=3):
        p = fake if ptrs else None
        return lib.vg_cluster_lshape(p, stride, p, p, n_clusters, criterion, p, n_angles, delta_zero, p, p, p, None)
    assert call(criterion=2) == VG_ERR_ARG
    assert call(criterion=-1) == VG_ERR_ARG
    assert call(n_angles=0) == VG_ERR_ARG
    assert call(n_angles=9002) == VG_ERR_ARG
    assert call(delta_zero=0.0) == VG_ERR_ARG
    assert call(delta_zero=-1.0) == VG_ERR_ARG
    assert call(delta_zero=float('nan')) == VG_ERR_ARG
    assert call(stride=2) == VG_ERR_ARG
    assert call(n_clusters=-1) == VG_ERR_ARG
    assert call(ptrs=False) == VG_ERR_ARG
    assert call(ptrs=False, criterion=1, delta_zero=0.0) == VG_ERR_ARG
    assert call(n_clusters=0, ptrs=False) == VG_OK                                  # a no-op
    assert call(n_clusters=0, ptrs=False, criterion=1, n_angles=9001, delta_zero=0.0) == VG_OK
    assert call(n_clusters=0, criterion=3) == VG_ERR_ARG


def test_lshape_kernels_hold_no_unencodable_64bit_literals():
    from vilgod_amd import build
    assert build.check_isa(sources=['lshape.hip']) == []
    assert build.check_scratch('lshape.hip', 'lshape') == []


def test_angle_tables():
    from vilgod_amd import boxes as vb
    c = vb.lshape_angle_table(*vb.box_method({'name': 'closeness_rectangle', 'args': {}}))
    v = vb.lshape_angle_table(*vb.box_method({'name': 'variance_rectangle', 'args': {}}))
    assert c.shape == (46, 8) and v.shape == (901, 8)
    for t, dt, delta in ((c, np.float32, 2), (v, np.float64, 0.1)):
        a = np.arange(0, 90 + delta, delta) / 180 * np.pi
        assert np.array_equal(t[:, 4], a) and np.array_equal(t[:, 5], a + np.pi / 2)
        assert np.array_equal(t[:, 6], a + np.pi / 2) and np.array_equal(t[:, 7], (a + np.pi / 2) + np.pi / 2)
        for k in (0, 1, len(a) // 3, len(a) - 1):
            assert t[k, 0] == dt(np.cos(a[k])) and t[k, 1] == dt(np.sin(a[k]))
            assert t[k, 2] == dt(np.cos(a[k] + np.pi / 2)) and t[k, 3] == dt(np.sin(a[k] + np.pi / 2))
    assert np.array_equal(c[:, :4], c[:, :4].astype(np.float32))
    assert vb.lshape_angle_table('variance_rectangle', {'delta': 0.01}).shape[0] == 9001
    with pytest.raises(ValueError):
        vb.lshape_angle_table('variance_rectangle', {'delta': 0.005})


def test_box_method_names_and_keywords():
    from vilgod_amd import boxes as vb
    from vilgod_amd import config as vconfig
    assert vb.box_method(None) == ('minimum_bounding_rectangle', {})
    assert vb.box_method({'name': 'closeness_rectangle', 'args': {}}) == ('closeness_rectangle', {'delta': 2, 'delta_zero': 1e-2})
    assert vb.box_method({'name': 'closeness_rectangle', 'args': {'delta': 1}}) == ('closeness_rectangle', {'delta': 1, 'delta_zero': 1e-2})
    assert vb.box_method(vconfig._wrap({'name': 'variance_rectangle', 'args': None})) == ('variance_rectangle', {'delta': 0.1})
    with pytest.raises(TypeError, match='delt'):
        vb.box_method({'name': 'variance_rectangle', 'args': {'delt': 0.2}})
    with pytest.raises(TypeError):
        vb.box_method({'name': 'variance_rectangle', 'args': {'delta_zero': 0.1}})
    with pytest.raises(TypeError):
        vb.box_method({'name': 'minimum_bounding_rectangle', 'args': {'delta': 2}})
    for bad in ('PCA_rectangle', 'closeness'):
        with pytest.raises(NotImplementedError, match='closeness_rectangle, variance_rectangle'):
            vb.box_method({'name': bad, 'args': {}})


def _stage_self(**kw):
    """The attributes fit_bounding_boxes_simple reads on a run without frames."""
    d = dict(tracker=None, my_frames=[], lidar_frame_list=[], _box_prefetch={}, _host_X={}, sync_lidar_frames=lambda: None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_stage_accepts_the_lshape_methods():
    from vilgod_amd.zero_shot_detector import ZeroShotDetector
    for m in ({'name': 'closeness_rectangle', 'args': {}}, {'name': 'closeness_rectangle', 'args': {'delta': 1, 'delta_zero': 0.05}},
              {'name': 'variance_rectangle', 'args': {'delta': 0.5}}, {'name': 'minimum_bounding_rectangle', 'args': {}}):
        ZeroShotDetector.fit_bounding_boxes_simple(_stage_self(), m, force=True, valid_only=True)
    with pytest.raises(NotImplementedError, match='variance_rectangle'):
        ZeroShotDetector.fit_bounding_boxes_simple(_stage_self(), {'name': 'PCA_rectangle', 'args': {}})
    with pytest.raises(TypeError):
        ZeroShotDetector.fit_bounding_boxes_simple(_stage_self(), {'name': 'closeness_rectangle', 'args': {'detla': 2}})


def _cfg(*overrides):
    from vilgod_amd import config as vconfig
    return vconfig.load(os.path.join(ROOT, 'tools', 'configs'), 'preprocessing', ['preprocessor=waymo'] + list(overrides))


def test_config_override_selects_the_method():
    cfg = _cfg('pipeline.6.args.method.name=closeness_rectangle', 'pipeline.6.args.method.args.delta=4')
    stage = cfg.pipeline[6]
    assert stage['name'] == 'fit_bounding_boxes_simple'
    from vilgod_amd.boxes import box_method
    assert box_method(stage['args']['method']) == ('closeness_rectangle', {'delta': 4, 'delta_zero': 1e-2})
    cfg = _cfg('pipeline.6.args.method.name=variance_rectangle')
    assert box_method(cfg.pipeline[6]['args']['method']) == ('variance_rectangle', {'delta': 0.1})


def test_classification_prefetches_min_area_rectangles_only():
    """box_mode='reference' sends the static min-area rectangles ahead during classification; that request knows no method, so an
    L-shape run must not make it (its boxes would be the min-area ones)."""
    from vilgod_amd.zero_shot_detector import ZeroShotDetector
    pipe = types.SimpleNamespace(box_mode='reference', mapped_names=['Background', 'Vehicle'], class_list=['car'])
    for override, want in (([], True), (['pipeline.6.args.method.name=closeness_rectangle'], False),
                           (['pipeline.6.args.method.name=variance_rectangle'], False)):
        cfg = _cfg(*override)
        me = types.SimpleNamespace(pipe=pipe, cfg=cfg)
        me._configured_box_method = types.MethodType(ZeroShotDetector._configured_box_method, me)
        assert ZeroShotDetector._classification_context(me)['prefetch_boxes'] is want


# ------------------------------------------------------------------------------------------- GPU
def _run(pipe_or_none, pts3, seg, name, args=None, cuda=None):
    """vg_cluster_lshape on packed clusters (pts3 [P,>=3] float32, seg offsets) -> (box [C,7], aux [C,3], work [C,A]) numpy."""
    import torch
    from vilgod_amd import boxes as vb
    from vilgod_amd._lib import lib, ptr, check
    name, args = vb.box_method({'name': name, 'args': args})
    tab = torch.from_numpy(vb.lshape_angle_table(name, args)).to(cuda)
    d_X = torch.from_numpy(np.ascontiguousarray(pts3, np.float32)).to(cuda)
    d_index = torch.arange(len(pts3), dtype=torch.int32, device=cuda)
    d_seg = torch.from_numpy(np.asarray(seg, np.int32)).to(cuda)
    C, A = len(seg) - 1, tab.shape[0]
    work = torch.empty((C, A), dtype=torch.float64, device=cuda)
    box = torch.empty((C, 7), dtype=torch.float64, device=cuda)
    aux = torch.empty((C, 3), dtype=torch.float64, device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.vg_cluster_lshape(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, vb.LSHAPE_METHODS[name][0], ptr(tab), A,
                                float(args.get('delta_zero', 1.0)), ptr(work), ptr(box), ptr(aux), stream), 'vg_cluster_lshape')
    torch.cuda.synchronize(cuda)
    return box.cpu().numpy(), aux.cpu().numpy(), work.cpu().numpy()


def _check_against(name, tol, clusters, box, aux, work, want_index, want_crit_for_ties, want_box=None, label=''):
    """same index: boxes within tol (and the restatement's criteria within 1e-9 relative); other index: a genuine near-tie of the
    compared criteria -> returns the number of near-ties."""
    ties = 0
    for c, p in enumerate(clusters):
        crit = lr.criteria_fast(p[:, :2], name)
        assert np.allclose(work[c], crit, rtol=1e-9, atol=1e-15), (label, c)
        k = int(aux[c, 0])
        assert aux[c, 1] == work[c].max() and k == int(np.flatnonzero(work[c] == work[c].max())[0])
        if k == want_index[c]:
            ref_box = want_box[c] if want_box is not None else lr.box(*lr.fit(p[:, :2], name, crit=work[c])[1:3], p[:, 2])
            assert np.allclose(box[c], ref_box, rtol=0, atol=tol), (label, c, box[c], ref_box)
        else:
            assert lr.near_tie(want_crit_for_ties[c], k, want_index[c], tol), (label, c, k, want_index[c])
            ties += 1
    return ties


@pytest.mark.gpu
@pytest.mark.parametrize('name,key,tol', METHODS)
def test_hip_lshape_matches_reference(cuda, golden, name, key, tol):
    cl = _clusters(golden)
    box, aux, work = _run(None, golden['points'], golden['seg'], name, cuda=cuda)
    ties = _check_against(name, tol, cl, box, aux, work, golden[f'{key}_index'], golden[f'{key}_crit'], golden[f'{key}_box'], 'golden')
    print(f'{name}: {ties} near-tie(s) of {len(cl)} golden clusters')
    assert ties <= 1
    for c, p in enumerate(cl):                                  # the chosen rectangle's orientation (before the l/w swap)
        if int(aux[c, 0]) == golden[f'{key}_index'][c]:
            assert aux[c, 2] == golden[f'{key}_angle'][c]
    box2, aux2, work2 = _run(None, golden['points'], golden['seg'], name, cuda=cuda)
    assert np.array_equal(box, box2, equal_nan=True) and np.array_equal(aux, aux2) and np.array_equal(work, work2)


@pytest.mark.gpu
@pytest.mark.parametrize('name,key,tol', METHODS)
def test_hip_lshape_real_and_random_clusters(cuda, golden_dir, name, key, tol):
    with open(f'{golden_dir}/detect_golden.pkl', 'rb') as f:
        g = pickle.load(f)
    gm = np.zeros(len(g['points']), bool)
    gm[g['ground_idx']] = True
    X = g['points_ref'][~gm][:, :3].astype(np.float32)
    real = [X[np.asarray(i)] for i in g['det_index']]
    rng = np.random.default_rng(7)
    rand = []
    for _ in range(2000):
        n = int(rng.integers(1, 200))
        kind = rng.integers(3)
        if kind == 0:
            xy = rng.normal(0, rng.uniform(0.05, 3), (n, 2)) * rng.uniform(0.2, 1, 2)
        elif kind == 1:
            t = rng.uniform(-0.5, 0.5, n)
            side = rng.integers(2, size=n)
            xy = np.where(side[:, None] == 0, np.stack([t * 4.5, np.full(n, -0.9)], 1), np.stack([np.full(n, 2.25), t * 1.8], 1))
            xy = xy + rng.normal(0, 0.03, (n, 2))
        else:
            xy = np.round(rng.uniform(-2, 2, (n, 2)), 1)                          # a coarse grid: many exact ties
        yaw = rng.uniform(-np.pi, np.pi)
        xy = xy @ np.array([[np.cos(yaw), np.sin(yaw)], [-np.sin(yaw), np.cos(yaw)]]) + rng.uniform(-50, 50, 2)
        rand.append(np.concatenate([xy, rng.uniform(-1, 2, (n, 1))], 1).astype(np.float32))
    ties_total = 0
    for label, cl in (('detect_golden', real), ('random', rand)):
        seg = np.r_[0, np.cumsum([len(p) for p in cl])]
        box, aux, work = _run(None, np.concatenate(cl), seg, name, cuda=cuda)
        want = [int(np.argmax(lr.criteria_fast(p[:, :2], name))) for p in cl]
        crits = [lr.criteria_fast(p[:, :2], name) for p in cl]
        ties = _check_against(name, tol, cl, box, aux, work, want, crits, None, label)
        print(f'{name} {label}: {ties} near-tie(s) of {len(cl)} clusters')
        ties_total += ties
    assert ties_total <= 5


@pytest.mark.gpu
def test_hip_lshape_through_the_pipeline(cuda, golden):
    """PseudoLabelPipeline.fit_boxes(method=...) == the entry point, in both box modes, with a gathered (index, seg) packing."""
    import torch
    from vilgod_amd.pipeline import PseudoLabelPipeline
    P, seg = golden['points'], golden['seg']
    pipe = PseudoLabelPipeline(device=cuda, max_points=len(P) + 16, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(P))                               # the points in another order; the index gathers them back
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(P))
    Xp = np.concatenate([P[perm], rng.uniform(-1, 1, (len(P), 2)).astype(np.float32)], 1)     # 5 columns like points_ref_wo_ground
    d_X = torch.from_numpy(np.ascontiguousarray(Xp)).to(cuda)
    index = inv.astype(np.int32)
    for name, key, tol in METHODS:
        want, _, _ = _run(None, P, seg, name, cuda=cuda)
        for mode in ('fast', 'reference'):
            pipe.box_mode = mode
            got = pipe.fit_boxes(d_X, index, seg, method={'name': name, 'args': {}})
            assert np.array_equal(got, want), (name, mode)


def _detector_run(tmp_path, tag, extra, stages=None):
    """tools/preprocess_data.py on a seeded synthetic sequence; the box stage is observed: per frame the boxes it wrote, the track
    flags, and vg_cluster_lshape's boxes of EVERY cluster of the frame (computed before the stage from the same device points)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    from vilgod_amd import zero_shot_detector as zmod
    from vilgod_amd.boxes import box_method, LSHAPE_METHODS
    seen = {}
    orig = zmod.ZeroShotDetector.fit_bounding_boxes_simple

    def observed(self, method, **kw):
        name, args = box_method(method)
        expect = {}
        if name in LSHAPE_METHODS:
            import torch
            for fs in self.lidar_frame_list:
                if fs.n_detections:
                    _, X = self._ref_and_nonground(fs.fnr)
                    d_index = torch.from_numpy(np.ascontiguousarray(fs.index, np.int32)).to(X.device)
                    d_seg = torch.from_numpy(np.ascontiguousarray(fs.seg_off, np.int32)).to(X.device)
                    expect[fs.fnr] = self.pipe.lshape_boxes(X, d_index, d_seg, name, args)[0].cpu().numpy()
        orig(self, method, **kw)
        for fs in self.lidar_frame_list:
            seen[fs.fnr] = (None if fs.boxes is None else fs.boxes.copy(), fs.static_track.copy(), expect.get(fs.fnr))
    zmod.ZeroShotDetector.fit_bounding_boxes_simple = observed
    try:
        ovr = ['dataset.SYNTHETIC.frames_per_sequence=6', 'dataset.SYNTHETIC.points_per_frame=20000',
               'dataset.SYNTHETIC.objects_per_frame=10', 'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0',
               'device.max_points=24000', 'paths.clip_model=/nonexistent']
        if stages:
            ovr.append('pipeline_active=[' + ','.join(stages) + ']')
        preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={tmp_path / tag}'] + ovr + list(extra))
    finally:
        zmod.ZeroShotDetector.fit_bounding_boxes_simple = orig
    return seen


@pytest.mark.gpu
def test_detector_uses_the_configured_lshape_method(cuda, tmp_path):
    base = _detector_run(tmp_path, 'mbr', [])
    n_static = n_moving = 0
    for name in ('closeness_rectangle', 'variance_rectangle'):
        run = _detector_run(tmp_path, name, [f'pipeline.6.args.method.name={name}'])
        assert sorted(run) == sorted(base)
        for fnr, (boxes, flags, expect) in run.items():
            bb, bflags, _ = base[fnr]
            assert np.array_equal(flags, bflags)                      # tracking does not depend on the boxes
            if boxes is None:
                continue
            for r in range(len(flags)):
                if flags[r] == 1:                                     # static track, or a track that turned out still
                    assert np.array_equal(boxes[r], expect[r]), (name, fnr, r)
                    n_static += 1
                elif flags[r] == 0:                                   # moving track: not the method's business
                    assert np.array_equal(boxes[r], bb[r], equal_nan=True), (name, fnr, r)
                    n_moving += 1
        if name == 'closeness_rectangle':
            fast = _detector_run(tmp_path, name + '_fast', [f'pipeline.6.args.method.name={name}', 'device.box_mode=fast'])
            for fnr, (boxes, flags, _) in run.items():
                fb = fast[fnr][0]
                assert (boxes is None) == (fb is None) and (boxes is None or np.array_equal(boxes, fb, equal_nan=True))
    print(f'{n_static} static-track boxes, {n_moving} moving-track boxes compared')
    assert n_static > 0 and n_moving > 0
    # without tracks (single-frame stage list): every boxed row is the kernel's box
    single = ['mask_ground_points', 'spatial_clustering', 'filter_detections', 'classification', 'fit_bounding_boxes_simple',
              'evaluate_sequence']
    run = _detector_run(tmp_path, 'variance_single', ['pipeline.6.args.method.name=variance_rectangle', 'pipeline.2.args.n_frames=1'],
                        stages=single)
    n = 0
    for fnr, (boxes, flags, expect) in run.items():
        if boxes is None:
            continue
        rows = np.flatnonzero(np.isfinite(boxes[:, 0]))
        assert np.array_equal(boxes[rows], expect[rows])
        n += len(rows)
    assert n > 0
