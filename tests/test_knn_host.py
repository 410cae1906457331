"""K nearest neighbours without a GPU: vg_knn_host (the kernel's pair function and order over all pairs), the walk's prune bound, the
numpy wrappers of vilgod_amd.knn through `search=knn_host`, and the kernel's scratch use.

Every comparison is exact: rows equal, squared distances equal as bit patterns.  The reference is tests/knn_ref.py: numpy over all
pairs, a lexicographic sort by (d2, row), the gate, the padding.
"""
import numpy as np
import pytest

import knn_ref as kr
import mst_ref as mr
import neighbors_ref as nr

F32 = np.float32
INF = np.inf


_lib, _p, host, switch_ks = kr._lib, kr._p, kr.host, kr.switch_ks


def _check(query, target, K, max_d2=INF):
    gi, gd = host(query, target, K, max_d2)
    msg = kr.same(gi, gd, *kr.knn(query, target, K, max_d2))
    assert not msg, f'K {K} max_d2 {max_d2!r}: {msg}'


# ================================================================================================ vg_knn_host == reference
@pytest.mark.parametrize('K', [1, 2, 3, 4, 5, 6, 7])
def test_ties(K):
    """groups of 2 to 6 targets at exactly equal d2: the row decides, also where K cuts through a group"""
    t, q, info = nr.ties()
    _check(q, t, K)
    _check(q, t, K, info['r2'])                                      # the gate exactly at the ties' distance: they all qualify
    _check(q, t, K, np.nextafter(info['r2'], F32(0)))                # ... one step below: none of them does


def test_ties_are_ties():
    """the scene holds what the tests above rely on: queries whose 2nd .. 6th neighbours are equidistant"""
    t, q, info = nr.ties()
    D, R, _ = kr.sorted_pairs(q, t)
    n = info['n_ring']
    same = (D[:n, :6] == info['r2']).sum(1)
    assert set(np.unique(same)) >= {2, 3, 4, 5, 6}


def test_dense_cell():
    t, q = nr.dense_cell()
    for K in switch_ks():
        _check(q, t, K)
    _check(q, t, 8, nr.R2_MOVING)


def test_outside_grid():
    t, q = nr.outside_grid()
    for K in (1, 4, 32):
        _check(q, t, K)
    for r2 in nr.RADII:
        _check(q, t, 5, r2)


@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_threshold_pairs(offset):
    """queries whose d2 to a target is the gate moved by -2 .. 2 float32 steps: <= keeps the pair at 0 and below"""
    t, q = nr.threshold_pairs(offset, nr.R2_GATE)
    for r2 in (nr.R2_GATE, np.nextafter(nr.R2_GATE, F32(0)), np.nextafter(nr.R2_GATE, F32(1))):
        _check(q, t, 1, r2)
        _check(q, t, 3, r2)
    _check(q, t, 9)


@pytest.mark.parametrize('K', [1, 5, 17, 32])
def test_few_targets(K):
    """M = 0, 1, 3, K - 1, K targets: the rest of each row is -1 / +inf"""
    t, q = nr.dense_cell()
    q = q[:64]
    for M in sorted({0, 1, 3, max(K - 1, 0), K}):
        tt = t[:M] if M else np.zeros((0, 4), F32)
        _check(q, tt, K)
        gi, gd = host(q, tt, K)
        assert (gi[:, M:] == -1).all() and np.isposinf(gd[:, M:]).all() and (gi[:, :M] >= 0).all()


def test_hundred_copies():
    """100 copies of one point: 32 rows at one distance, lowest rows first"""
    t = np.repeat(F32([[3.25, -1.5, 0.75, 0.0]]), 100, 0)
    q = F32([[3.25, -1.5, 0.75], [3.0, -1.5, 0.75], [40.0, 2.0, 1.0]])
    for K in switch_ks():
        _check(q, t, K)
        gi, gd = host(q, t, K)
        assert np.array_equal(gi, np.tile(np.arange(K), (3, 1))) and (gd[0] == 0).all()


def test_nonfinite_queries():
    t, q = nr.dense_cell()
    qq = kr.nonfinite_rows(q)
    bad = ~np.isfinite(qq).all(1)
    assert bad.sum() >= 10 and (~bad).sum() >= 10
    for K in (1, 4, 9):
        for r2 in (INF, 0.5):
            _check(qq, t, K, r2)
            gi, gd = host(qq, t, K, r2)
            assert (gi[bad] == -1).all() and np.isposinf(gd[bad]).all()


def test_strides():
    """qstride 5 (and target rows of 4 floats): the columns behind z are never read"""
    t, q = nr.outside_grid()
    q5 = np.c_[q, np.full((len(q), 2), np.nan, F32)].astype(F32)
    gi, gd = host(q5, t, 6)
    assert q5.shape[1] == 5 and t.shape[1] == 4
    assert not kr.same(gi, gd, *kr.knn(q, t, 6))


def test_refusals():
    lib = _lib()
    q, t = np.zeros((2, 3), F32), np.ones((4, 3), F32)
    idx, d2 = np.zeros((2, 32), np.int32), np.zeros((2, 32), F32)
    from vilgod_amd.knn import KNN_MAX_K
    call = lambda nq=2, qs=3, nt=4, ts=3, K=1, r2=INF, pq=q, pt=t, pi=idx, pd=d2: lib.vg_knn_host(_p(pq), nq, qs, _p(pt), nt, ts, K, r2, _p(pi), _p(pd))
    assert call() == 0
    assert call(K=KNN_MAX_K) == 0
    for kw in (dict(K=0), dict(K=-1), dict(K=KNN_MAX_K + 1), dict(qs=2), dict(ts=2), dict(r2=0.0), dict(r2=-1.0), dict(r2=float('nan')),
               dict(nq=-1), dict(nt=-1), dict(pq=None), dict(pi=None), dict(pd=None), dict(pt=None)):
        assert call(**kw) == 1, kw
    assert call(nq=0, pq=None, pi=None, pd=None) == 0                # nothing to do
    assert call(nt=0, pt=None) == 0 and (idx.reshape(-1)[:2] == -1).all()      # no targets: every entry ([2, 1]) missing


# ================================================================================================ the prune bound
def _face_pairs(origin):
    """(points, queries) float32 [m,3]: along each axis the point 0, +-1, +-2 float32 steps from a face (every 7th face, the first and last
    ones, and clamped beyond the grid), the query the neighbouring values on either side, 0.3 .. 60 m away and beyond the grid; the other
    two coordinates equal -- the axis distance is the whole distance, the sharpest case -- or one float32 step apart."""
    P, Q = [], []
    for a in range(3):
        faces = np.unique(np.r_[0, 1, 2, np.arange(3, mr.NB[a], 7), mr.NB[a] - 2, mr.NB[a] - 1, mr.NB[a]])
        v = np.unique(np.concatenate([mr.face_values(origin, a, faces), mr.outside_values(origin, a)]))
        m, j = len(v), np.arange(len(v))
        qs = [v[np.clip(j + s, 0, m - 1)] for s in range(-5, 6)]
        qs += [(v.astype(np.float64) + d).astype(F32) for d in (-60.0, -7.0, -1.1, -0.3, 0.3, 1.1, 7.0, 60.0)]
        qs += [np.full(m, o, F32) for o in mr.outside_values(origin, a)]
        q = np.stack(qs, 1)
        p = np.repeat(v[:, None], q.shape[1], 1)
        b, c = (a + 1) % 3, (a + 2) % 3
        for variant in range(2):
            pp, qq = np.zeros(p.shape + (3,), F32), np.zeros(p.shape + (3,), F32)
            pp[..., a], qq[..., a] = p, q
            fb = F32(origin[b] + 100.5 * mr.CELL)
            pp[..., b], qq[..., b] = fb, (fb if variant == 0 else mr.steps(fb, 1))
            pp[..., c] = qq[..., c] = F32(origin[c] + 30.5 * mr.CELL)
            P.append(pp.reshape(-1, 3)); Q.append(qq.reshape(-1, 3))
    return np.concatenate(P), np.concatenate(Q)


def _bound(box_d2):
    f = _lib().vg_knn_prune_bound_host
    return np.array([f(float(v)) for v in np.unique(box_d2)]), np.unique(box_d2, return_inverse=True)[1]


def test_prune_bound_is_below_the_float32_distance():
    """d2_f32(q, p) >= prune_bound(box_d2(q, node_l(p))) for l = 0 .. 6: a node the walk skips holds no target the list would take.
    box_d2 comes from vg_cluster_geom_probe (the functions the kernel calls), never from a restatement."""
    origins = [mr.probe(points=np.zeros((1, 3), F32), bbox=(F32(a) - F32([30, 30, 3]), F32(a) + F32([30, 30, 3])))['origin'] for a in nr.OFFSETS]
    assert any(abs(o[0] - 1000) < 150 for o in origins)              # the origin around (1000, 1000, 0)
    origins += [nr.face_lattice(o)[2] for o in nr.OFFSETS[:2]]
    total = below = sharp = 0
    for origin in origins:
        P, Q = _face_pairs(origin)
        r = mr.probe(points=P, queries=Q, origin=origin, want_code=False)
        d32 = nr.d2_f32(Q, P).astype(np.float64)
        vals, inv = _bound(r['box_d2'])
        bound = vals[inv.reshape(-1)].reshape(r['box_d2'].shape)
        bad = np.argwhere(bound > d32[:, None])
        assert len(bad) == 0, (origin.tolist(), P[bad[0][0]].tolist(), Q[bad[0][0]].tolist(), int(bad[0][1]), float(bound[tuple(bad[0])]), float(d32[bad[0][0]]))
        total += bound.size
        under = d32 < nr.d2_exact(Q, P)
        below += int(under.sum())
        sharp += int((under[:, None] & (r['box_d2'] > d32[:, None])).sum())     # the float64 bound alone would have skipped a target here
    print(f'{total} triples, {below} pairs with float32 d2 below the float64 distance, {sharp} triples where box_d2 itself exceeds the float32 d2')
    assert total > 500_000 and below > 1000 and sharp > 0


def test_prune_bound_in_the_subnormal_range():
    """a face at exactly 0.0 (origin -0.8, face 2), the point on it, the query 1e-22 below: the float32 d2 is 7 subnormal steps
    (9.8e-45) and lies BELOW box_d2 = 1e-44 by more than any relative slack covers"""
    origin = np.array([-0.8, -0.8, -0.8])
    P, Q = F32([[0.0, 0.1, 0.1]]), F32([[-1e-22, 0.1, 0.1]])
    r = mr.probe(points=P, queries=Q, origin=origin, want_code=False)
    d32 = float(nr.d2_f32(Q, P)[0])
    assert 0 < d32 < 1.2e-38 and r['box_d2'][0, 0] > d32 > 0.9 * r['box_d2'][0, 0]
    f = _lib().vg_knn_prune_bound_host
    assert all(f(float(b)) <= d32 for b in r['box_d2'][0])
    # and the bound stays a bound worth having: within 1e-6 (relative) of the box distance wherever that is not tiny
    for b in (1e-6, 0.16, 25.0, 1e6):
        assert b * (1 - 1e-6) < f(b) < b
    assert f(0.0) <= 0.0


# ================================================================================================ the numpy wrappers
def _wrapper_scene():
    t, q = nr.dense_cell()
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, 40, len(t)).astype(np.int64)
    probs = rng.random(len(t))
    return q[:300], t, labels, probs


@pytest.mark.parametrize('N', [300, 2, 1])
@pytest.mark.parametrize('K', [1, 4])
def test_knn_wrapper_shapes_and_values(N, K):
    from vilgod_amd import knn as vk
    q, t, _, _ = _wrapper_scene()
    d, i = vk.knn(q[:N], t, K=K, search=vk.knn_host)
    wd, wi = kr.restated_knn(q[:N], t, K=K)
    want_shape = tuple(s for s in (N, K) if s != 1)
    assert d.shape == i.shape == wd.shape == want_shape
    assert d.dtype == np.float32 and i.dtype == np.int64
    assert np.array_equal(i, wi) and np.array_equal(d.view(np.int32), wd.view(np.int32))


@pytest.mark.parametrize('N', [300, 1])
@pytest.mark.parametrize('thr', [0.2, 0.01])
def test_knn_labels_wrapper(N, thr):
    from vilgod_amd import knn as vk
    q, t, labels, probs = _wrapper_scene()
    gl, gp = vk.knn_labels(q[:N], t, labels, probs, dist_threshold=thr, search=vk.knn_host)
    wl, wp = kr.restated_knn_labels(q[:N], t, labels, probs, dist_threshold=thr)
    assert np.array_equal(np.asarray(gl), np.asarray(wl)) and np.array_equal(gp, wp)
    assert type(gl) is type(wl)
    if N > 1:                                                        # (one point and K > 1: the reference's `if dists > ...` has no truth value)
        assert (gl == -1).any() and (gl >= 0).any()
        gl, gp = vk.knn_labels(q[:N], t, labels, K=3, search=vk.knn_host)
        wl, _ = kr.restated_knn_labels(q[:N], t, labels, K=3)
        assert gp is None and np.array_equal(gl, wl) and np.shape(gl) == np.shape(wl) == (N, 3)


@pytest.mark.parametrize('smallest_first', [True, False])
def test_chamfer_wrapper(smallest_first):
    from vilgod_amd import knn as vk
    q, t, _, _ = _wrapper_scene()
    a, b = t[:, :3], (q + F32(0.05))
    for p1, p2 in ((a, b), (b, a), (a[:1], b), (a, a)):
        got = vk.chamfer_distance(p1, p2, smallest_first=smallest_first, threshold=0.2, search=vk.knn_host)
        want = kr.restated_chamfer(p1, p2, smallest_first=smallest_first, threshold=0.2)
        assert type(got) is type(want) and got.dtype == np.float32
        assert np.array_equal(np.float32(got).view(np.int32), np.float32(want).view(np.int32))
    assert vk.chamfer_distance(a, a, search=vk.knn_host) == 0


def test_wrappers_refuse_an_empty_target_set():
    from vilgod_amd import knn as vk
    q, t, labels, _ = _wrapper_scene()
    none = np.zeros((0, 3), F32)
    with pytest.raises(ValueError):
        vk.knn(q, none, search=vk.knn_host)
    with pytest.raises(ValueError):
        vk.knn_labels(q, none, labels[:0], search=vk.knn_host)
    with pytest.raises(ValueError):
        vk.chamfer_distance(q, none, search=vk.knn_host)


def test_knn_points_refuses_what_it_does_not_implement():
    """the argument checks come before any GPU work"""
    import torch
    from vilgod_amd import knn as vk
    p = torch.zeros((1, 4, 3))
    with pytest.raises(NotImplementedError, match='norm'):
        vk.knn_points(p, p, norm=1)
    with pytest.raises(NotImplementedError, match='p2'):
        vk.knn_points(p, torch.zeros((1, 4, 2)))
    with pytest.raises(ValueError, match='float32'):
        vk.knn_points(p.double(), p)
    with pytest.raises(ValueError, match='CUDA'):
        vk.knn_points(p, p)
    with pytest.raises(ValueError):
        vk.knn_points(p.numpy(), p)


# ================================================================================================ the kernel's resources
def test_kernel_uses_no_scratch():
    from vilgod_amd import build
    assert build.check_scratch('cluster.hip', 'k_cl_knn') == []
    import re
    names = set(re.findall(r'\.set (\S*k_cl_knn\S*)\.private_seg_size', build._device_asm('cluster.hip')))
    assert len(names) == 5, names                                    # every instantiation was looked at
