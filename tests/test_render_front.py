"""The renderer's front end -- k_gather_ego, k_cluster_median's view angle and rotation row, k_cluster_rot, k_to_origin of
csrc/render.hip -- against exact arithmetic (tests/render_front_ref.py).

CPU: the numpy restatements of the four kernels are tied to exact values (Fraction for the affine maps, mpmath for atan2 / sin / cos),
to the reference's own frozen outputs and to scipy, so that the GPU part can demand bits of the kernels.
GPU: every comparison is either bitwise against such a restatement, or the bar max(8 * E_host, 2^-50) against mpmath for the rotation
entries (E_host = the host-libm restatement's own worst error, measured by the CPU part; the device's sin / cos need not return
glibc's bits).  Run with `pytest -s` for the measured figures.
"""
import ctypes

import numpy as np
import pytest
import torch

import render_front_ref as R

VG_OK, VG_ERR_ARG = 0, 1
AMBIGUOUS_CAP = 1e-4                  # share of a seeded input that may lie within the float64 error of a float32 rounding midpoint
CANARY32 = np.uint32(0xC0DEC0DE)
CANARY64 = np.uint64(0xC0DEC0DEC0DEC0DE)
N_CANARY = 3
TIMG_PERM = np.array([[0., -1., 0.], [-1., 0., 0.], [0., 0., -1.]])      # Timg without scipy's 1e-16 entries: exact 0 / +-1


def _check_exact(name, got, want, amb):
    """got == want bit for bit where the exact value is not ambiguous, within one float32 step where it is"""
    share = float(amb.mean())
    print(f'{name}: {int(amb.sum())}/{amb.size} values ambiguous (share {share:.2e}), '
          f'{int((R.bits(got) != R.bits(want)).sum())} differ from the correctly rounded exact value')
    assert share <= AMBIGUOUS_CAP, name
    assert np.array_equal(R.bits(got)[~amb], R.bits(want)[~amb]), name
    assert (R.f32_steps(got, want)[amb] <= 1).all(), name


def _origin_case(n=4000, seed=23):
    """points around the seeded medians, every cluster with the rotation row of its own (libm) view angle"""
    rng = np.random.default_rng(seed)
    med = R.seeded_medians()
    c = rng.integers(0, len(med), n).astype(np.int32)
    ego = (med[c] + rng.normal(size=(n, 3)) * np.abs(med[c])).astype(np.float32)
    ang = np.arctan2(med[:, 1].astype(np.float64), med[:, 0].astype(np.float64)).astype(np.float32)
    return ego, c, med, R.view_rotation(ang)


# ------------------------------------------------------------------------------------------------------------------------- CPU
def test_render_hip_is_built_without_contraction():
    """what makes a numpy restatement a bitwise bar: only the FMAs written in render.hip exist (none in the front end)"""
    from vilgod_amd import build
    assert build.SOURCES['render.hip'] == ['-ffp-contract=off']


def test_gather_ego_restatement_is_the_correctly_rounded_exact_value():
    p, T = R.big_pose_points(), R.big_pose()
    want, amb = R.exact_gather_ego(p, 5, None, T)
    _check_exact('gather_ego, large-translation pose', R.gather_ego(p, 5, None, T), want, amb)
    assert np.abs(want[:, :2]).min() > 1000                      # the pose leaves large coordinates: float32 steps of ~1e-3
    idx = np.random.default_rng(1).permutation(len(p))[:500]
    want, amb = R.exact_gather_ego(p, 5, idx, R.translation_pose())
    _check_exact('gather_ego, pure translation', R.gather_ego(p, 5, idx, R.translation_pose()), want, amb)


def test_to_origin_restatement_is_the_correctly_rounded_exact_value():
    ego, c, med, rot = _origin_case()
    for name, timg in (('scipy', R.timg()), ('permutation', TIMG_PERM)):
        want, amb = R.exact_to_origin(ego, c, med, rot, timg)
        _check_exact(f'to_origin, 4000 seeded medians, Timg {name}', R.to_origin(ego, c, med, rot, timg), want, amb)


def test_float64_atan2_rounds_to_the_correctly_rounded_view_angle():
    """what the kernel evaluates, float32(atan2(double, double)), on the host: the inputs of the GPU test are not ambiguous"""
    import math
    m = R.seeded_medians()
    want, amb = R.exact_atan2(m[:, 1], m[:, 0])
    got = np.array([math.atan2(float(y), float(x)) for y, x in zip(m[:, 1], m[:, 0])]).astype(np.float32)
    _check_exact('view angle, 4000 seeded medians', got, want, amb)
    assert np.abs(m).min() >= 1e-7 and np.abs(m).max() > 80 and (np.abs(m) < 1e-2).any()


def test_to_origin_restatement_equals_the_reference_outputs(golden_dir):
    """On the golden clusters the restatement, cast to float32, is the reference's own `originf32_i` bit for bit -- what
    test_hip_origin_and_median_match_oracle demands of the kernel.  The reference's angle is numpy's float32 arctan2 on the host that
    wrote the fixture, a <= 1 ulp routine: it is one of the correctly rounded angle and its two float32 neighbours."""
    g = np.load(f'{golden_dir}/render_golden.npz')
    n_cases = g['hashes'].shape[0]
    assert n_cases == 12
    for i in range(n_cases):
        c = g[f'pts_{i}']
        assert c.dtype == np.float32
        med = np.median(c, axis=0)[None]
        exact, amb = R.exact_atan2(med[:, 1], med[:, 0])
        hits = [a for a in R.neighbours(exact[0])
                if R.same_bits(R.to_origin(c, np.zeros(len(c), np.int64), med, R.view_rotation([a]), R.timg()), g[f'originf32_{i}'])]
        assert len(hits) == 1, i
        if f'origin_{i}' in g:                                   # the reference's float64 output: the cast is the only step between
            assert R.same_bits(g[f'origin_{i}'].astype(np.float32), g[f'originf32_{i}'])


def test_view_rotation_restatement_equals_scipy_and_has_a_measured_error():
    from scipy.spatial.transform import Rotation
    ang = R.rotation_angles()
    assert len(ang) >= 100_000 and ang.dtype == np.float32 and np.abs(ang).max() == R.neighbours(R.PI32)[2]
    edge = R.edge_angles()
    for v in (0.0, np.pi, np.pi / 2):
        for s in (1, -1):
            w = np.float32(s * v)
            for nb in R.neighbours(w) if v else [w]:
                assert (R.bits(edge) == R.bits(nb)).any(), (w, nb)
    assert np.float32(1e-30) in edge and R.TINY32 in edge
    rows, e_host = R.host_rotation()
    m = Rotation.from_euler('z', -ang).as_matrix()                                # float32 negation, like the reference's `-angle`
    assert (-ang).dtype == np.float32
    want = np.stack([m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1], m[:, 2, 2]], axis=1)
    assert np.array_equal(rows[:, :5], want)                                      # as numbers
    assert np.array_equal(m[:, 2, :2], np.zeros((len(ang), 2))) and np.array_equal(m[:, :2, 2], np.zeros((len(ang), 2)))
    assert np.array_equal(rows[:, 5], ang.astype(np.float64))
    _check_rotation_structure(rows)
    assert (rows[:, 5] == 0).sum() == 2
    print(f'view_rotation with the host libm on {len(ang)} angles: E_host = {e_host:.3e}, bar max(8 E_host, 2^-50) = {R.rotation_bar(e_host):.3e}')
    assert 0 < e_host <= 2.0 ** -50                               # a few float64 roundings of values <= 1


def test_front_end_entry_points_check_arguments():
    """no device work: every call returns before a launch (fake non-null pointers are never dereferenced).  An empty call is VG_OK
    whatever else it is given; a NULL d_index is no error (the stride < 3 call below fails on its stride: with a valid stride and a
    NULL index the GPU tests get VG_OK)."""
    from vilgod_amd._lib import lib
    fake = ctypes.c_void_p(16)

    def gather(n=1, stride=3, null=None, index=fake):
        p = [fake if null != k else None for k in range(3)]
        return lib.vg_gather_ego(p[0], stride, index, n, p[1], p[2], None)
    assert gather(n=0) == VG_OK and gather(n=-1) == VG_OK
    assert gather(n=0, stride=2, null=0, index=None) == VG_OK
    assert lib.vg_gather_ego(None, 0, None, 0, None, None, None) == VG_OK
    for stride in (2, 0, -1):
        assert gather(stride=stride) == VG_ERR_ARG
        assert gather(stride=stride, index=None) == VG_ERR_ARG
    for k in range(3):
        assert gather(null=k) == VG_ERR_ARG
        assert gather(null=k, index=None) == VG_ERR_ARG

    def median(n=1, null=None):
        p = [fake if null != k else None for k in range(4)]
        return lib.vg_cluster_median(p[0], p[1], n, p[2], p[3], None)
    assert median(n=0) == VG_OK and median(n=-1) == VG_OK and lib.vg_cluster_median(None, None, 0, None, None, None) == VG_OK
    for k in range(4):
        assert median(null=k) == VG_ERR_ARG

    def rot(n=1, null=None):
        p = [fake if null != k else None for k in range(2)]
        return lib.vg_cluster_rot(p[0], n, p[1], None)
    assert rot(n=0) == VG_OK and rot(n=-1) == VG_OK and lib.vg_cluster_rot(None, 0, None, None) == VG_OK
    for k in range(2):
        assert rot(null=k) == VG_ERR_ARG

    def origin(n=1, null=None):
        p = [fake if null != k else None for k in range(6)]
        return lib.vg_to_origin(p[0], p[1], n, p[2], p[3], p[4], p[5], None)
    assert origin(n=0) == VG_OK and origin(n=-1) == VG_OK and lib.vg_to_origin(None, None, 0, None, None, None, None, None) == VG_OK
    for k in range(6):
        assert origin(null=k) == VG_ERR_ARG


def _check_rotation_structure(rows):
    """true of the formula whatever sin / cos return"""
    assert np.array_equal(R.bits(rows[:, 0]), R.bits(rows[:, 3]))                 # m00 == m11
    assert np.array_equal(R.bits(rows[:, 1]), R.bits(-rows[:, 2]))                # m01 == -m10
    zero = rows[:, 5] == 0
    assert np.array_equal(rows[zero][:, :5], np.tile([1., 0., 0., 1., 1.], (int(zero.sum()), 1)))


# ------------------------------------------------------------------------------------------------------------------------- GPU
def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)                 # a copy: some inputs are read-only


def _out(rows, cols, dtype, cuda):
    """an output buffer of `rows` rows with N_CANARY canary rows behind them, every word the canary"""
    word = CANARY32 if dtype == np.float32 else CANARY64
    return _dev(np.full((rows + N_CANARY, cols), word).view(dtype), cuda)


def _read(t, rows):
    """-> the first `rows` rows; the canary rows behind them must have survived"""
    a = t.cpu().numpy()
    word = CANARY32 if a.dtype == np.float32 else CANARY64
    assert (R.bits(a[rows:]) == word).all(), 'canary rows overwritten'
    assert len(a) == rows + N_CANARY
    return a[:rows]


def _run_gather(cuda, pts, stride, idx, n, T):
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    d_pts, d_T = _dev(pts, cuda), _dev(np.asarray(T, np.float64), cuda)
    d_idx = None if idx is None else _dev(idx.astype(np.int32), cuda)
    ego = _out(n, 3, np.float32, cuda)
    check(lib.vg_gather_ego(ptr(d_pts), stride, ptr(d_idx), n, ptr(d_T), ptr(ego), stream_ptr()), 'vg_gather_ego')
    return _read(ego, n)


def _run_median(cuda, ego, seg_off):
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    C = len(seg_off) - 1
    d_ego, d_seg = _dev(ego.astype(np.float32), cuda), _dev(np.asarray(seg_off, np.int32), cuda)
    med, rot = _out(C, 3, np.float32, cuda), _out(C, 6, np.float64, cuda)
    check(lib.vg_cluster_median(ptr(d_ego), ptr(d_seg), C, ptr(med), ptr(rot), stream_ptr()), 'vg_cluster_median')
    return _read(med, C), _read(rot, C)


def _run_rot(cuda, ang):
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    d_ang = _dev(np.asarray(ang, np.float32), cuda)
    rot = _out(len(ang), 6, np.float64, cuda)
    check(lib.vg_cluster_rot(ptr(d_ang), len(ang), ptr(rot), stream_ptr()), 'vg_cluster_rot')
    return _read(rot, len(ang))


def _run_origin(cuda, ego, c, med, rot, timg):
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    n = len(ego)
    d = [_dev(ego.astype(np.float32), cuda), _dev(c.astype(np.int32), cuda), _dev(med.astype(np.float32), cuda),
         _dev(np.asarray(rot, np.float64), cuda), _dev(np.asarray(timg, np.float64), cuda)]
    out = _out(n, 3, np.float32, cuda)
    check(lib.vg_to_origin(ptr(d[0]), ptr(d[1]), n, ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(out), stream_ptr()), 'vg_to_origin')
    return _read(out, n)


@pytest.mark.gpu
@pytest.mark.parametrize('stride', [3, 4, 5, 7])
def test_hip_gather_ego_equals_the_restatement_bit_for_bit(cuda, stride):
    rng = np.random.default_rng(100 + stride)
    for n in (1, 255, 256, 257, 1000):
        rows = n + 5                                              # rows the NULL index never reaches
        for pose, T in (('identity', np.eye(4)), ('translation', R.translation_pose()), ('large', R.big_pose())):
            pts = np.full((rows, stride), np.nan, np.float32)     # NaN in the unused columns
            if pose == 'large':
                pts[:, :3] = (np.array(R.BIG_CENTRE) + rng.uniform(-40, 40, (rows, 3))).astype(np.float32)
            else:
                pts[:, :3] = (rng.normal(size=(rows, 3)) * 30).astype(np.float32)
                pts[0, :3] = [R.SUB32, -R.TINY32, np.float32(3e38)]                  # a flushed subnormal shows
            repeats = rng.integers(0, rows, n + 2)
            repeats[:3] = [rows - 1, 0, 0]                        # the last row, and row 0 twice
            for kind, idx in (('null', None), ('permutation', rng.permutation(rows)[:n]), ('repeats', repeats[:n])):
                got = _run_gather(cuda, pts, stride, idx, n, T)
                taken = np.arange(n) if idx is None else idx      # a NULL index is the first n rows
                assert R.same_bits(got, R.gather_ego(pts, stride, taken, T)), (n, pose, kind)
                if pose == 'identity':                            # no -0 among the inputs: x * 1 + 0 + 0 + 0 keeps every other value
                    assert R.same_bits(got, np.ascontiguousarray(pts[taken, :3])), (n, kind)


# (med_y, med_x) -> the float32 view angle
ANGLE_TABLE = [
    ((0.0, 1.0), 0.0), ((-0.0, 1.0), -0.0), ((0.0, -1.0), R.PI32), ((-0.0, -1.0), -R.PI32),
    ((1.0, 0.0), R.HALF_PI32), ((1.0, -0.0), R.HALF_PI32), ((-1.0, 0.0), -R.HALF_PI32), ((-1.0, -0.0), -R.HALF_PI32),
    ((0.0, 0.0), 0.0), ((-0.0, 0.0), -0.0), ((0.0, -0.0), R.PI32), ((-0.0, -0.0), -R.PI32),
    ((np.float32(1e-20), 1.0), np.float32(1e-20)), ((R.SUB32, 1.0), R.SUB32), ((np.float32(1e-30), np.float32(1e30)), 0.0),
]


def _table_clusters():
    """one-point clusters of ANGLE_TABLE with an empty cluster in the middle -> (ego [P,3], seg_off [C+1], expected angle [C], row of
    the empty cluster)"""
    ego = np.array([[x, y, 0.5 * (k + 1)] for k, ((y, x), _) in enumerate(ANGLE_TABLE)], np.float32)
    want = np.array([a for _, a in ANGLE_TABLE], np.float32)
    empty = 7
    seg = np.concatenate([np.arange(empty + 1), np.arange(empty, len(ego) + 1)])
    return ego, seg, np.insert(want, empty, np.float32(0.0)), empty


def _check_rotation_rows(rows, what):
    """structure, and every entry within the bar of the mpmath value -> the worst error"""
    _, e_host = R.host_rotation()
    _check_rotation_structure(rows)
    worst = float(R.rotation_error(rows).max())
    assert worst <= R.rotation_bar(e_host), (what, worst, e_host)
    return worst


@pytest.mark.gpu
def test_hip_cluster_median_angle_at_the_edges(cuda):
    """axes, signed zeros, +-pi, a subnormal angle, an underflowing one, and the empty cluster's `n > 0 ? ... : 0` branch"""
    ego, seg, want, empty = _table_clusters()
    med, rot = _run_median(cuda, ego, seg)
    keep = np.arange(len(want)) != empty
    assert R.same_bits(med[keep], ego)                            # one point: the median is the point, signed zeros included
    assert R.same_bits(med[empty], np.zeros(3, np.float32))
    got = rot[:, 5].astype(np.float32)
    assert np.array_equal(got.astype(np.float64), rot[:, 5])
    for k in range(len(want)):
        assert R.bits(got[k:k + 1])[0] == R.bits(want[k:k + 1])[0], (k, got[k], want[k])
    assert float(R.SUB32) in rot[:, 5]                            # the subnormal is not flushed
    assert np.array_equal(rot[empty], [1., 0., 0., 1., 1., 0.])
    _check_rotation_rows(rot, 'edge table')


def _check_angles(name, med, rot):
    got = rot[:, 5].astype(np.float32)
    assert np.array_equal(got.astype(np.float64), rot[:, 5])      # rot[:, 5] is a float32 value
    want, amb = R.exact_atan2(med[:, 1], med[:, 0])
    _check_exact(name, got, want, amb)


@pytest.mark.gpu
def test_hip_cluster_median_angle_is_correctly_rounded_on_seeded_medians(cuda):
    m = R.seeded_medians()
    med, rot = _run_median(cuda, m, np.arange(len(m) + 1))
    assert R.same_bits(med, m)
    _check_angles('device view angle, 4000 seeded medians', med, rot)
    _check_rotation_rows(rot, 'seeded medians')


@pytest.mark.gpu
def test_hip_cluster_median_1025_clusters(cuda):
    """more clusters than any block-sized table: clusters of 1 .. 4 points, np.median semantics"""
    m = R.seeded_medians()
    sizes = np.arange(1025) % 4 + 1
    seg = np.concatenate([[0], np.cumsum(sizes)])
    ego = m[:seg[-1]]
    want = np.stack([np.median(ego[seg[k]:seg[k + 1]], axis=0) for k in range(1025)])
    assert want.dtype == np.float32 and (want[:, :2] != 0).all()
    med, rot = _run_median(cuda, ego, seg)
    assert R.same_bits(med, want)
    _check_angles('device view angle, 1025 clusters', med, rot)
    _check_rotation_rows(rot, '1025 clusters')


@pytest.mark.gpu
def test_hip_rotation_rows_of_both_entry_points(cuda):
    ang = R.rotation_angles()
    host, e_host = R.host_rotation()
    for n in (1, 63, 64, 65):
        rows = _run_rot(cuda, ang[:n])
        assert np.array_equal(rows[:, 5], ang[:n].astype(np.float64))
        assert float(R.rotation_error(rows).max()) <= R.rotation_bar(e_host), n
    rows = _run_rot(cuda, ang)
    assert R.same_bits(rows[:65], _run_rot(cuda, ang[:65]))
    assert R.same_bits(rows[:, 5], ang.astype(np.float64))
    worst = _check_rotation_rows(rows, 'vg_cluster_rot')
    differ = int((R.bits(rows) != R.bits(host)).any(axis=1).sum())
    print(f'rotation rows on {len(ang)} angles: device worst error {worst:.3e}, E_host {e_host:.3e}, bar {R.rotation_bar(e_host):.3e}; '
          f'{differ} rows differ in bits from the host-libm restatement')
    # the same angles through vg_cluster_median: the edge table's and the seeded medians' own angles
    ego, seg, _, _ = _table_clusters()
    m = R.seeded_medians()
    seg = np.concatenate([seg, seg[-1] + 1 + np.arange(len(m))])
    _, via_median = _run_median(cuda, np.concatenate([ego, m]), seg)
    _check_rotation_rows(via_median, 'vg_cluster_median')
    via_rot = _run_rot(cuda, via_median[:, 5].astype(np.float32))
    assert R.same_bits(via_median, via_rot)
    zeros = via_median[via_median[:, 5] == 0]
    assert len(zeros) >= 5 and np.signbit(zeros[:, 5]).any() and not np.signbit(zeros[:, 5]).all()


def _origin_inputs(rng, n, C):
    """unsorted cluster ids with repeats; medians with +-0; a point equal to its median (x and y cancel to 0) and a point a float32
    subnormal away from it; rotation rows of the edge angles"""
    med = (rng.normal(size=(C, 3)) * 10.0 ** rng.uniform(-3, 1.9, (C, 1))).astype(np.float32)
    tiny = min(1, C - 1)
    if C > 1:
        med[0] = [0.0, -0.0, 1.5]
        med[tiny] = [2e-38, -2e-38, 0.25]
    else:                                                         # one cluster: its x stays an ordinary value (an inexact float32 difference)
        med[0, 1:] = [-2e-38, 0.25]
    c = rng.integers(0, C, n).astype(np.int32)
    c[-1] = C - 1
    c[0] = tiny
    if n > 2:
        c[1], c[2] = 0, tiny
    ego = (med[c] + rng.normal(size=(n, 3))).astype(np.float32)
    ego[0, 1:] = [-2.5e-38, 0.75]                                 # differences of +-5e-39: float32 subnormals
    if C > 1:
        ego[0, 0] = 2.5e-38
    if n > 2:
        ego[1] = [-0.0, 0.0, -2.0]
        ego[2] = med[tiny]
    rot = R.view_rotation(R.edge_angles())[np.arange(C) % len(R.edge_angles())]
    return ego, c, med, rot


@pytest.mark.gpu
@pytest.mark.parametrize('C', [1, 7, 1025])
def test_hip_to_origin_equals_the_restatement_bit_for_bit(cuda, C):
    rng = np.random.default_rng(300 + C)
    for n in (1, 255, 256, 257, 5000):
        ego, c, med, rot = _origin_inputs(rng, n, C)
        if n > 2:
            x64 = ego[:, 0].astype(np.float64) - med[c, 0].astype(np.float64)
            assert (x64 != (ego[:, 0] - med[c, 0]).astype(np.float64)).any()          # the float32 subtraction rounds somewhere
            assert len(np.unique(c)) < n and c.max() == C - 1 and c.min() == 0 and (C == 1 or (np.diff(c) < 0).any())
        for name, timg in (('scipy', R.timg()), ('permutation', TIMG_PERM)):
            want = R.to_origin(ego, c, med, rot, timg)
            if name == 'permutation':                             # a flushed subnormal difference or result would show
                assert ((want != 0) & (np.abs(want) < 2.0 ** -126)).any(), (n, C)
            got = _run_origin(cuda, ego, c, med, rot, timg)
            assert np.array_equal(got, want), (n, C, name, int((got != want).sum()))        # as numbers: -0.0 == 0.0


def _stage_frame(seed=400):
    """~300 clusters of 10 .. 3000 points around BIG_CENTRE in a stride-5 array, gathered through a shuffled index"""
    rng = np.random.default_rng(seed)
    sizes = (10 * 300.0 ** (rng.uniform(0, 1, 300) ** 4)).astype(np.int64)
    sizes[:2] = [10, 3000]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ptot = int(seg[-1])
    assert sizes.min() == 10 and sizes.max() == 3000 and 20_000 <= ptot <= 60_000
    centre = np.array(R.BIG_CENTRE) + rng.uniform(-40, 40, (300, 3))
    xyz = np.repeat(centre, sizes, axis=0) + rng.normal(size=(ptot, 3)) * [0.5, 1.0, 0.3]
    rows = ptot + 1000                                            # rows no cluster owns lie between them
    index = rng.permutation(rows)[:ptot].astype(np.int32)
    pts = np.full((rows, 5), np.nan, np.float32)
    pts[:, :3] = rng.normal(size=(rows, 3)).astype(np.float32)
    pts[index, :3] = xyz.astype(np.float32)
    return pts, index, seg


@pytest.mark.gpu
@pytest.mark.parametrize('angle_mode', ['device', 'reference'])
def test_hip_front_end_as_render_frame_runs_it(cuda, angle_mode):
    from vilgod_amd.projection import RealisticProjection
    pts, index, seg = _stage_frame()
    T = R.big_pose()
    d_pts, d_index, d_seg = _dev(pts, cuda), _dev(index, cuda), _dev(seg, cuda)
    proj = RealisticProjection({}, device=cuda, angle_mode=angle_mode)

    def run(stream):
        torch.cuda.synchronize()
        img = proj.render_frame(d_pts, d_index, d_seg, T, out='raw110', stream=stream)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in dict(proj._last, img=img).items()}
    got = run(None)
    want_ego = R.gather_ego(pts, 5, index, T)
    assert R.same_bits(got['ego'], want_ego)
    want_med = np.stack([np.median(want_ego[seg[k]:seg[k + 1]], axis=0) for k in range(len(seg) - 1)])
    assert R.same_bits(got['median'], want_med)
    ang = got['rot'][:, 5].astype(np.float32)
    assert np.array_equal(ang.astype(np.float64), got['rot'][:, 5])
    exact, amb = R.exact_atan2(want_med[:, 1], want_med[:, 0])
    if angle_mode == 'device':
        _check_exact('device view angle, 300 clusters', ang, exact, amb)
    else:                                                         # this host's numpy float32 arctan2, a <= 1 ulp routine
        assert R.same_bits(ang, np.arctan2(want_med[:, 1], want_med[:, 0]))
        assert float(amb.mean()) <= AMBIGUOUS_CAP and (R.f32_steps(ang, exact) <= 1).all()
    _check_rotation_rows(got['rot'], angle_mode)
    want = R.to_origin(got['ego'], R.point_clusters(seg), got['median'], got['rot'], R.timg())
    assert R.same_bits(got['origin'], want)
    side = run(torch.cuda.Stream(device=cuda))
    for k in got:
        assert R.same_bits(side[k], got[k]), k
