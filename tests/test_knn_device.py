"""K nearest neighbours on the GPU: vg_cluster_knn (k_cl_knn, csrc/cluster_knn.inc) equals vg_knn_host equals the dense numpy reference
of tests/knn_ref.py -- rows equal, squared distances equal as bit patterns, no tolerance anywhere -- and agrees with the two fixed-radius
kernels it generalises; then the layers above it: HDBSCAN.knn on a reused handle, knn_points, and the numpy wrappers.
"""
import numpy as np
import pytest

import knn_ref as kr
import neighbors_ref as nr

F32 = np.float32
INF = np.inf
host, switch_ks = kr.host, kr.switch_ks
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(cuda):
    from vilgod_amd.hdbscan import HDBSCAN
    return HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15, max_points=8192)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(model, cuda, q, K, max_d2=INF):
    idx, d2 = model.knn(_dev(q, cuda), K, max_d2)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _check(model, cuda, q, t, K, max_d2=INF, grid=True):
    """kernel == vg_knn_host == reference for one (scene, K, gate); grid=False: the handle's grid already holds t"""
    if grid:
        model.grid(_dev(t, cuda))
    gi, gd = _run(model, cuda, q, K, max_d2)
    wi, wd = kr.knn(q, t, K, max_d2)
    msg = kr.same(gi, gd, wi, wd)
    assert not msg, f'kernel vs reference, K {K} max_d2 {max_d2!r}: {msg}'
    hi, hd = host(q, t, K, max_d2)
    msg = kr.same(gi, gd, hi.astype(np.int64), hd)
    assert not msg, f'kernel vs vg_knn_host, K {K} max_d2 {max_d2!r}: {msg}'


def _gates(r2):
    r2 = F32(r2)
    return [np.nextafter(r2, F32(0)), r2, np.nextafter(r2, F32(np.inf))]


# ================================================================================================ kernel == host == reference
@pytest.mark.parametrize('order', [0, 1, 2])
def test_ties(cuda, model, order):
    """2 to 6 equidistant targets in up to six cells: the row decides, in three target orders (the reference is recomputed per order)"""
    t, q, info = nr.ties()
    t = t[kr.orders(len(t))[order]]
    model.grid(_dev(t, cuda))
    for K in (1, 2, 3, 4, 5, 6, 7):
        _check(model, cuda, q, t, K, grid=False)
    for g in _gates(info['r2']):
        _check(model, cuda, q, t, 4, g, grid=False)
        _check(model, cuda, q, t, 7, g, grid=False)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_dense_cell(cuda, model, order):
    """3 000 targets in one cell and its neighbours: every instantiation of the kernel, K on both sides of every switch point"""
    t, q = nr.dense_cell()
    t = t[kr.orders(len(t))[order]]
    model.grid(_dev(t, cuda))
    for K in switch_ks():
        _check(model, cuda, q, t, K, grid=False)
    for g in _gates(nr.R2_MOVING):
        _check(model, cuda, q, t, 8, g, grid=False)
        _check(model, cuda, q, t, 17, g, grid=False)


@pytest.mark.parametrize('order', [0, 2])
def test_outside_grid(cuda, model, order):
    """targets and queries beyond the grid on every side (clamped into border cells)"""
    t, q = nr.outside_grid()
    t = t[kr.orders(len(t))[order]]
    model.grid(_dev(t, cuda))
    for K in (1, 4, 9, 32):
        _check(model, cuda, q, t, K, grid=False)
    for r2 in nr.RADII:
        for g in _gates(r2):
            _check(model, cuda, q, t, 5, g, grid=False)


@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_threshold_pairs(cuda, model, offset):
    """pairs whose d2 is the gate moved by -2 .. 2 float32 steps, gates at the radius and one step either side"""
    t, q = nr.threshold_pairs(offset, nr.R2_GATE)
    model.grid(_dev(t, cuda))
    for g in _gates(nr.R2_GATE):
        _check(model, cuda, q, t, 1, g, grid=False)
        _check(model, cuda, q, t, 3, g, grid=False)
    _check(model, cuda, q, t, 9, grid=False)


@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_face_lattice(cuda, model, offset):
    """targets on, and one float32 step either side of, cell faces, edges and corners; queries at the radius across them"""
    t, q, _ = nr.face_lattice(offset)
    model.grid(_dev(t, cuda))
    for K in (1, 2, 5, 16):
        _check(model, cuda, q, t, K, grid=False)
    for g in _gates(nr.R2_ENTROPY):
        _check(model, cuda, q, t, 2, g, grid=False)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_sparse_scene_crosses_roots(cuda, model, order):
    """40 targets over 200 m, every query 50 .. 150 m from all of them, K = 32: the walk leaves its root and still returns everything"""
    t, q = kr.sparse()
    t = t[kr.orders(len(t))[order]]
    _check(model, cuda, q, t, 32)
    gi, _ = _run(model, cuda, q, 32)
    assert (gi >= 0).all() and all(len(set(r)) == 32 for r in gi)
    _check(model, cuda, q, t, 1, grid=False)
    _check(model, cuda, q, t, 32, F32(100.0 ** 2), grid=False)        # a gate that cuts the lists short


@pytest.mark.parametrize('K', [1, 5, 17, 32])
def test_few_targets(cuda, model, K):
    """M = 0, 1, 3, K - 1, K targets"""
    t, q = nr.dense_cell()
    for M in sorted({0, 1, 3, K - 1, K}):
        _check(model, cuda, q[:200], t[:M] if M else np.zeros((0, 4), F32), K)


def test_hundred_copies(cuda, model):
    t = np.repeat(F32([[3.25, -1.5, 0.75, 0.0]]), 100, 0)
    q = F32([[3.25, -1.5, 0.75], [3.0, -1.5, 0.75], [40.0, 2.0, 1.0]])
    model.grid(_dev(t, cuda))
    for K in switch_ks():
        _check(model, cuda, q, t, K, grid=False)


def test_nonfinite_queries_and_strides(cuda, model):
    """query rows with NaN / +-inf get -1 / +inf in all K places; rows of 5 floats: the columns behind z are not read, rows past nq
    are not written"""
    import torch
    t, q = nr.dense_cell()
    qq = kr.nonfinite_rows(q)
    bad = ~np.isfinite(qq).all(1)
    model.grid(_dev(t, cuda))
    for K in (1, 4, 9, 32):
        for g in (INF, 0.5):
            _check(model, cuda, qq, t, K, g, grid=False)
        gi, gd = _run(model, cuda, qq, K)
        assert (gi[bad] == -1).all() and np.isposinf(gd[bad]).all() and (gi[~bad] >= 0).all()
    for nq in (1, 127, 128, 129, 255, 256, 257):                     # one block and the next, for both block sizes
        q5 = np.full((nq, 5), np.nan, F32)
        q5[:, :3] = q[:nq]
        for K in (4, 9):
            idx = torch.full((nq + 8, K), -7, dtype=torch.int32, device=cuda)
            d2 = torch.full((nq + 8, K), -7.0, dtype=torch.float32, device=cuda)
            model.knn(_dev(q5, cuda), K, out=(idx[:nq], d2[:nq]))
            assert not kr.same(idx[:nq].cpu().numpy(), d2[:nq].cpu().numpy(), *kr.knn(q[:nq], t, K)), (nq, K)
            assert int((idx[nq:] != -7).sum()) == 0 and int((d2[nq:] != -7.0).sum()) == 0


def test_refusals(cuda, model):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    from vilgod_amd.knn import KNN_MAX_K
    t, q = nr.dense_cell()
    dt, dq = _dev(t, cuda), _dev(q, cuda)
    model.grid(dt)
    idx = torch.full((len(q), KNN_MAX_K), -7, dtype=torch.int32, device=cuda)
    d2 = torch.full((len(q), KNN_MAX_K), -7.0, dtype=torch.float32, device=cuda)
    call = lambda nq=len(q), qs=3, K=1, r2=INF, pq=dq, pi=idx, pd=d2: lib.vg_cluster_knn(model._h, ptr(pq), nq, qs, K, r2, ptr(pi), ptr(pd), stream_ptr())
    for kw in (dict(K=0), dict(K=-1), dict(K=KNN_MAX_K + 1), dict(qs=2), dict(r2=0.0), dict(r2=-1.0), dict(r2=float('nan')), dict(nq=-1),
               dict(pq=None), dict(pi=None), dict(pd=None)):
        assert call(**kw) == 1, kw
    assert call(nq=0, pq=None, pi=None, pd=None) == 0
    torch.cuda.synchronize()
    assert int((idx != -7).sum()) == 0 and int((d2 != -7.0).sum()) == 0          # refused: nothing written
    assert call(K=KNN_MAX_K) == 0
    assert not kr.same(idx.cpu().numpy(), d2.cpu().numpy(), *kr.knn(q, t, KNN_MAX_K))


# ================================================================================================ against the existing kernels
@pytest.mark.parametrize('name', ['ties', 'dense', 'outside', 'lattice'])
def test_k1_with_a_gate_equals_nearest(cuda, model, name):
    """K = 1 with a gate == vg_cluster_nearest, row and bits, at every gate the latter accepts (it refuses gates past 8 cells)"""
    t, q = {'ties': lambda: nr.ties()[:2], 'dense': nr.dense_cell, 'outside': nr.outside_grid, 'lattice': lambda: nr.face_lattice(nr.OFFSETS[1])[:2]}[name]()
    dq = _dev(q, cuda)
    model.grid(_dev(t, cuda))
    for g in nr.RADII + (nr.R2_KNN, nr.R2_REACH1, nr.R2_REACH2, nr.R2_REACH8):
        ni, nd = (x.cpu().numpy() for x in model.nearest(dq, g))
        ki, kd = (x.cpu().numpy() for x in model.knn(dq, 1, g))
        assert np.array_equal(ki[:, 0], ni) and np.array_equal(kd[:, 0].view(np.int32), nd.view(np.int32)), (name, g)


def test_moving_point_mask_equals_ball_count(cuda, model):
    """zero_shot_detector.py:221-222 through knn() equals the ball_count form the two-frame clusterer uses"""
    from vilgod_amd import knn as vk
    mp = kr.moving_points()
    dmp = _dev(mp, cuda)
    model.grid(dmp)
    want = (model.ball_count(dmp, np.float32(0.1), 4) - 1 >= 2).cpu().numpy()
    got = np.sum(vk.knn(mp, mp, 4)[0][:, 1:] < 0.1, axis=1) > 1
    assert np.array_equal(got, want) and 200 < got.sum() < len(mp) - 200


class _MadeUpTree:
    """An HDBSCAN handle whose clustering is replaced by made-up labels: TwoFrameClusterer.labels then runs its own label transfer
    (grid over the clustering input, `nearest` within the gate, gather) on the real kernels."""

    def __init__(self, model, labels, probs, cuda):
        self._m, self._lab, self._prob, self.hierarchy, self._cuda = model, labels, probs, 'host', cuda

    def __getattr__(self, k):
        return getattr(self._m, k)

    def mst(self, seq, dim=3):
        import torch
        e = torch.empty(0, device=self._cuda)
        return e, e, e

    def tree(self, lo, hi, w2, n):
        return self._lab.astype(np.int32), self._prob, 10


def test_knn_labels_equals_the_two_frame_label_transfer(cuda, model):
    from vilgod_amd import knn as vk
    from vilgod_amd.entropy import TwoFrameClusterer
    t, q = nr.outside_grid()
    rng = np.random.default_rng(5)
    labels, probs = rng.integers(0, 10, len(t)), rng.random(len(t))
    two = TwoFrameClusterer(_MadeUpTree(model, labels, probs, cuda), n_frames=2, seed=0)
    dseq = _dev(np.c_[t, np.zeros(len(t), F32)].astype(F32), cuda)
    two.cluster_input = lambda fnr, X_list, ent_list: dseq
    dq = _dev(np.c_[q, np.ones(len(q), F32)].astype(F32), cuda)
    wl, wp = two.labels(1, [dq, dq], [None, None])
    gl, gp = vk.knn_labels(q, t, labels, probs)
    assert np.array_equal(gl, wl) and (gl == -1).sum() >= 100 and (gl >= 0).sum() >= 100
    assert np.array_equal(gp[gl >= 0], wp[gl >= 0])                  # (the reference keeps the probability of a gated neighbour; labels() zeroes it)


# ================================================================================================ one handle, many uses
def test_handle_reuse(cuda):
    """grid -> knn -> mst -> grid of another size -> knn on ONE handle: nothing of an earlier use may remain"""
    from vilgod_amd.hdbscan import HDBSCAN
    m = HDBSCAN(min_cluster_size=5, max_points=4096)
    t, q = nr.dense_cell()
    _check(m, cuda, q, t, 9)
    x = _dev(kr.moving_points(1500, seed=2), cuda)
    lo, hi, w2 = m.mst(x)
    assert lo.numel() == 1499
    # (the MST left ITS points in the grid: the search runs against them)
    xi, xd = (v.cpu().numpy() for v in m.knn(x, 3))
    assert not kr.same(xi, xd, *kr.knn(x.cpu().numpy(), x.cpu().numpy(), 3))
    t2, q2 = nr.outside_grid()
    _check(m, cuda, q2, t2[:777], 9)
    _check(m, cuda, q, t, 32)
    lo2, hi2, w22 = m.mst(x)
    # ... and the search left the handle fit for the next tree: the same weights, the same edge set (equal weights come in any order)
    edges = lambda a, b: sorted(zip(a.cpu().tolist(), b.cpu().tolist()))
    assert np.array_equal(w22.cpu().numpy(), w2.cpu().numpy()) and edges(lo2, hi2) == edges(lo, hi)


# ================================================================================================ knn_points
def _ragged(cuda):
    rng = np.random.default_rng(9)
    t, q = nr.dense_cell()
    t2, q2 = nr.outside_grid()
    P1, P2 = 400, 900
    p1 = np.stack([q[:P1], q2[:P1], q[100:100 + P1]]).astype(F32)
    p2 = np.stack([t[:P2, :3], t2[:P2, :3], t[rng.permutation(len(t))[:P2], :3]]).astype(F32)
    return p1, p2, [400, 257, 1], [900, 333, 3]


def _check_points(res, p1, p2, l1, l2, K):
    d, i = res.dists.cpu().numpy(), res.idx.cpu().numpy()
    assert d.shape == i.shape == (len(p1), p1.shape[1], K) and d.dtype == np.float32 and i.dtype == np.int64
    for b in range(len(p1)):
        msg = kr.same(i[b, :l1[b]], d[b, :l1[b]], *kr.knn(p1[b, :l1[b]], p2[b, :l2[b]], K))
        assert not msg, (b, msg)
        assert (i[b, l1[b]:] == -1).all() and np.isposinf(d[b, l1[b]:]).all()
        assert (i[b, :l1[b], min(K, l2[b]):] == -1).all()


@pytest.mark.parametrize('K', [1, 5])
def test_knn_points_ragged_batch(cuda, K):
    """B = 3, ragged lengths, an element with lengths2 = 3 < K = 5; lengths as lists and as tensors; return_nn"""
    import torch
    from vilgod_amd import knn as vk
    p1, p2, l1, l2 = _ragged(cuda)
    d1, d2 = _dev(p1, cuda), _dev(p2, cuda)
    res = vk.knn_points(d1, d2, lengths1=l1, lengths2=l2, K=K)
    assert res.knn is None and tuple(res._fields) == ('dists', 'idx', 'knn')
    _check_points(res, p1, p2, l1, l2, K)
    res = vk.knn_points(d1, d2, lengths1=torch.tensor(l1, device=cuda), lengths2=torch.tensor(l2, device=cuda), K=K, return_nn=True)
    _check_points(res, p1, p2, l1, l2, K)
    i, nn = res.idx.cpu().numpy(), res.knn.cpu().numpy()
    assert nn.shape == i.shape + (3,)
    for b in range(3):
        assert np.array_equal(nn[b], np.where((i[b] >= 0)[..., None], p2[b][np.maximum(i[b], 0)], 0))
    full = vk.knn_points(d1, d2, K=K)                                # no lengths: every row
    _check_points(full, p1, p2, [p1.shape[1]] * 3, [p2.shape[1]] * 3, K)


def test_knn_points_shared_model_and_growing_cache(cuda, model):
    import torch
    from vilgod_amd import knn as vk
    p1, p2, l1, l2 = _ragged(cuda)
    d1, d2 = _dev(p1, cuda), _dev(p2, cuda)
    # a caller's handle: used, not replaced, and no cached one is made for it
    before = dict(vk._handles)
    res = vk.knn_points(d1, d2, lengths1=l1, lengths2=l2, K=3, model=model)
    _check_points(res, p1, p2, l1, l2, 3)
    assert vk._handles == before
    with pytest.raises(Exception):                                   # more targets than the caller's handle holds: an error, no silent second handle
        vk.knn_points(d1[:1], torch.zeros((1, model.max_points + 1, 3), device=cuda), model=model)
    # the cached handle: made on first use, kept, replaced by a larger one when a larger target set arrives
    old_min, vk._MIN_HANDLE_POINTS = vk._MIN_HANDLE_POINTS, 512
    try:
        vk._handles.clear()
        _check_points(vk.knn_points(d1, d2[:, :300], K=2), p1, p2[:, :300], [400] * 3, [300] * 3, 2)
        h0 = vk._handles[cuda.index]
        assert h0.max_points == 512
        _check_points(vk.knn_points(d1, d2[:, :500], K=2), p1, p2[:, :500], [400] * 3, [500] * 3, 2)
        assert vk._handles[cuda.index] is h0
        _check_points(vk.knn_points(d1, d2, K=2), p1, p2, [400] * 3, [900] * 3, 2)
        h1 = vk._handles[cuda.index]
        assert h1 is not h0 and h1.max_points >= 900
        _check_points(vk.knn_points(d1, d2[:, :300], K=2), p1, p2[:, :300], [400] * 3, [300] * 3, 2)      # smaller again: the larger handle stays
        assert vk._handles[cuda.index] is h1
    finally:
        vk._MIN_HANDLE_POINTS = old_min
        vk._handles.clear()


# ================================================================================================ the numpy wrappers on the GPU
def test_wrappers_equal_their_host_forms(cuda):
    from vilgod_amd import knn as vk
    t, q = nr.dense_cell()
    rng = np.random.default_rng(3)
    labels, probs = rng.integers(-1, 40, len(t)).astype(np.int64), rng.random(len(t))
    bits = lambda a: np.asarray(a, F32).view(np.int32)
    for N in (300, 1):
        for K in (1, 4):
            gd, gi = vk.knn(q[:N], t, K=K)
            hd, hi = vk.knn(q[:N], t, K=K, search=vk.knn_host)
            assert gd.shape == hd.shape and gi.shape == hi.shape and gi.dtype == hi.dtype == np.int64
            assert np.array_equal(gi, hi) and np.array_equal(bits(gd), bits(hd))
        for thr in (0.2, 0.01):
            gl, gp = vk.knn_labels(q[:N], t, labels, probs, dist_threshold=thr)
            hl, hp = vk.knn_labels(q[:N], t, labels, probs, dist_threshold=thr, search=vk.knn_host)
            assert type(gl) is type(hl) and np.array_equal(gl, hl) and np.array_equal(gp, hp)
    a, b = t[:, :3], q + F32(0.05)
    for p1, p2 in ((a, b), (b, a), (a[:1], b)):
        for sf in (True, False):
            g, h = vk.chamfer_distance(p1, p2, smallest_first=sf), vk.chamfer_distance(p1, p2, smallest_first=sf, search=vk.knn_host)
            assert type(g) is type(h) and np.array_equal(bits(g), bits(h))
    with pytest.raises(ValueError):
        vk.knn(q, np.zeros((0, 3), F32))
