"""Ball query on the GPU: vg_cluster_ball_query (k_cl_ball_query, csrc/cluster_ball_query.inc) equals vg_ball_query_host equals the dense
numpy reference of tests/ball_query_ref.py -- every entry of idx and cnt equal, no tolerance anywhere --, cnt equals
vg_cluster_ball_count with cap = nsample, and the guard rows around idx / cnt stay untouched; then the layers above it: ball_query() on
ragged batches, shared and cached handles, a captured graph, the count wrappers.
"""
import numpy as np
import pytest

import ball_query_ref as br
import neighbors_ref as nr

F32 = np.float32
GUARD = 3                                                     # rows of poison in front of and behind idx / cnt
POISON = -7
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def model(cuda):
    from vilgod_amd.cluster_handle import GridQueries
    return GridQueries(1 << 17, cuda)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(model, cuda, dq, nsample, r2, want_cnt=True):
    """one launch into the middle of poisoned buffers -> (idx, cnt) on the host, the guard rows checked"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    nq = dq.shape[0]
    idx = torch.full((nq + 2 * GUARD, nsample), POISON, dtype=torch.int32, device=cuda)
    cnt = torch.full((nq + 2 * GUARD,), POISON, dtype=torch.int32, device=cuda)
    if want_cnt:
        model.ball_query(dq, r2, nsample, out=(idx[GUARD:GUARD + nq], cnt[GUARD:GUARD + nq]))
    else:
        check(lib.vg_cluster_ball_query(model._h, ptr(dq), nq, dq.stride(0) if nq else 3, float(F32(r2)), nsample, ptr(idx[GUARD:]), None,
                                        stream_ptr()), 'vg_cluster_ball_query')
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    assert (idx[:GUARD] == POISON).all() and (idx[GUARD + nq:] == POISON).all(), 'idx: guard rows written'
    assert (cnt[:GUARD] == POISON).all() and (cnt[GUARD + nq:] == POISON).all(), 'cnt: guard rows written'
    return idx[GUARD:GUARD + nq], cnt[GUARD:GUARD + nq]


def _check(model, cuda, q, t, r2, nsample, d2=None, dq=None):
    """kernel == vg_ball_query_host == reference and cnt == ball_count(cap = nsample), for the grid the handle holds (built over t)"""
    dq = _dev(q, cuda) if dq is None else dq
    gi, gc = _run(model, cuda, dq, nsample, r2)
    wi, wc = br.from_d2(br.d2_matrix(q, t) if d2 is None else d2, r2, nsample)
    msg = br.same(gi, gc, wi, wc)
    assert not msg, f'kernel vs reference, r2 {r2!r} nsample {nsample}: {msg}'
    msg = br.same(gi, gc, *br.host(q, t, r2, nsample))
    assert not msg, f'kernel vs vg_ball_query_host, r2 {r2!r} nsample {nsample}: {msg}'
    bc = model.ball_count(dq, r2, nsample).cpu().numpy()
    assert np.array_equal(gc, bc), f'cnt vs vg_cluster_ball_count, r2 {r2!r} nsample {nsample}: {int((gc != bc).sum())} differ'
    return gi, gc


def _scene(model, cuda, q, t, cases, order=0):
    """one scene in one target order: the grid and the pair distances once, then every (r2, nsample) of `cases`"""
    t = t[br.orders(len(t))[order]]
    model.grid(_dev(t, cuda))
    dq, d2 = _dev(q, cuda), br.d2_matrix(q, t)
    return [_check(model, cuda, q, t, r2, nsample, d2, dq) for r2, nsample in cases]


# ================================================================================================ kernel == host == reference
@pytest.mark.parametrize('order', [0, 1, 2])
@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_threshold_pairs(cuda, model, offset, order):
    """pairs 0, +-1, +-2 float32 steps from the radius, at the four radii the reference project uses"""
    for r2 in nr.RADII:
        t, q = nr.threshold_pairs(offset, r2)
        _scene(model, cuda, q, t, [(r2, 1), (r2, 3), (r2, 100)], order)


@pytest.mark.parametrize('order', [0, 1, 2])
@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_face_lattice(cuda, model, offset, order):
    t, q, _ = nr.face_lattice(offset)
    _scene(model, cuda, q, t, [(nr.R2_ENTROPY, 1), (nr.R2_ENTROPY, 4), (nr.R2_ENTROPY, 100)], order)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_outside_grid(cuda, model, order):
    """queries and targets beyond the grid on every side (clamped into border cells)"""
    t, q = nr.outside_grid()
    _scene(model, cuda, q, t, [(r2, 16) for r2 in nr.RADII] + [(nr.R2_REACH2, 1000)], order)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_ties(cuda, model, order):
    """equidistant hits in different cells come out by row; at r2 == d2 exactly none of them is a hit"""
    t, q, info = nr.ties()
    above = np.nextafter(info['r2'], F32(np.inf))
    (_, c1), (_, c2), (_, c0) = _scene(model, cuda, q, t, [(above, 8), (above, 3), (info['r2'], 8)], order)
    assert c1[:info['n_ring']].min() >= 2 and c1.max() >= 6 and c2.max() == 3 and (c0[:info['n_ring']] == 0).all()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_dense_cell(cuda, model, order):
    """0 .. 873, 0 .. 1 901 and 2 153 .. 3 003 hits per query: below, around and above the wave's buffer, at every nsample"""
    t, q = nr.dense_cell()
    _scene(model, cuda, q, t, [(r2, n) for r2 in br.DENSE_R2 for n in br.NSAMPLES], order)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_hit_counts_around_the_buffer_size(cuda, model, order):
    """one query with exactly C - 1, C, C + 1, 2 C, 2 C + 1 hits (C = VG_BALL_QUERY_CAND) and C - 65, C - 64, C - 63 (the fill at
    which the kernel cuts); as built, the nsample lowest rows lie in the cell the kernel scans last"""
    C = br.cand()
    for hits in (C - 65, C - 64, C - 63, C - 1, C, C + 1, 2 * C, 2 * C + 1):
        for nsample in (1, 1023, 1024):
            t, q = br.built(hits, nsample)
            (gi, gc), = _scene(model, cuda, q, t, [(nr.R2_ENTROPY, nsample)], order)
            if order == 0:
                assert gc[0] == min(hits, nsample) and np.array_equal(gi[0, :gc[0]], np.arange(gc[0]))


@pytest.mark.parametrize('interleaved', [False, True])
def test_many_coincident_targets(cuda, model, interleaved):
    """40 000 copies of one point (one cell, every row a hit): the answer is the first nsample copies' rows"""
    t, q = br.coincident(interleaved)
    step = 2 if interleaved else 1
    for order in (0, 1):
        for (gi, gc), nsample in zip(_scene(model, cuda, q, t, [(nr.R2_ENTROPY, 1000), (nr.R2_ENTROPY, 1)], order), (1000, 1)):
            first = np.arange(nsample) * step + (1 if interleaved and order == 1 else 0)      # (reversed: the copies sit on the odd rows)
            assert (gc == nsample).all() and (gi == first).all()


def test_reach_limits(cuda, model):
    """r2 = 10.24 is 8 cells, the last reach taken; one float32 step above is refused and idx keeps its poison"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    t, q = nr.reach_limits()
    (gi, gc), _ = _scene(model, cuda, q, t, [(nr.R2_REACH8, 1024), (nr.R2_REACH8, 5)])
    assert gc.min() >= 100
    dq = _dev(q, cuda)
    idx = torch.full((len(q), 5), POISON, dtype=torch.int32, device=cuda)
    cnt = torch.full((len(q),), POISON, dtype=torch.int32, device=cuda)
    above = float(np.nextafter(nr.R2_REACH8, F32(np.inf)))
    assert lib.vg_cluster_ball_query(model._h, ptr(dq), len(q), 3, above, 5, ptr(idx), ptr(cnt), stream_ptr()) == 1
    torch.cuda.synchronize()
    assert int((idx != POISON).sum()) == 0 and int((cnt != POISON).sum()) == 0


def test_empty_and_degenerate_inputs(cuda, model):
    import torch
    t, q = nr.dense_cell()
    # an empty grid: zeros, cnt = 0
    model.grid(torch.zeros((0, 4), device=cuda))
    gi, gc = _run(model, cuda, _dev(q, cuda), 9, nr.R2_ENTROPY)
    assert (gi == 0).all() and (gc == 0).all()
    # no queries
    model.grid(_dev(t, cuda))
    gi, gc = _run(model, cuda, torch.zeros((0, 3), device=cuda), 9, nr.R2_ENTROPY)
    assert gi.shape == (0, 9)
    # queries that are not points, between good ones
    qq = br.nonfinite_rows(q)
    bad = ~np.isfinite(qq).all(1)
    for nsample in (1, 9, 100):
        gi, gc = _check(model, cuda, qq, t, nr.R2_ENTROPY, nsample)
        assert (gc[bad] == 0).all() and (gi[bad] == 0).all() and (gc[~bad] > 0).any()
    # floats per query row 3 / 4 / 7: the columns behind z are not read; nq on both sides of a workgroup's four queries
    for w in (3, 4, 7):
        for nq in (1, 3, 4, 5, 257):
            qw = np.full((nq, w), np.nan, F32)
            qw[:, :3] = q[:nq]
            gi, gc = _run(model, cuda, _dev(qw, cuda), 7, nr.R2_ENTROPY)
            assert not br.same(gi, gc, *br.ball_query(q[:nq], t, nr.R2_ENTROPY, 7)), (w, nq)


def test_null_cnt_still_writes_idx(cuda, model):
    t, q = nr.dense_cell()
    model.grid(_dev(t, cuda))
    gi, gc = _run(model, cuda, _dev(q, cuda), 65, F32(0.2), want_cnt=False)
    assert (gc == POISON).all() and not br.same(gi, None, *br.ball_query(q, t, F32(0.2), 65))


def test_refusals(cuda, model):
    """every refusal returns VG_ERR_ARG and leaves the outputs as they were"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    from vilgod_amd.ball_query import BALL_QUERY_MAX_NSAMPLE as MAXN
    t, q = nr.dense_cell()
    dq = _dev(q, cuda)
    model.grid(_dev(t, cuda))
    idx = torch.full((len(q), MAXN), POISON, dtype=torch.int32, device=cuda)
    cnt = torch.full((len(q),), POISON, dtype=torch.int32, device=cuda)
    call = lambda nq=len(q), qs=3, n=4, r2=0.09, pq=dq, pi=idx, pc=cnt, h=model._h: lib.vg_cluster_ball_query(h, ptr(pq), nq, qs, r2, n, ptr(pi), ptr(pc),
                                                                                                                stream_ptr())
    for kw in (dict(n=0), dict(n=-1), dict(n=MAXN + 1), dict(qs=2), dict(r2=0.0), dict(r2=-1.0), dict(r2=float('nan')), dict(r2=float('inf')),
               dict(r2=10.25), dict(nq=-1), dict(pq=None), dict(pi=None), dict(h=None)):
        assert call(**kw) == 1, kw
    assert call(nq=0, pq=None, pi=None, pc=None) == 0
    torch.cuda.synchronize()
    assert int((idx != POISON).sum()) == 0 and int((cnt != POISON).sum()) == 0
    assert call(n=MAXN) == 0
    assert not br.same(idx.cpu().numpy(), cnt.cpu().numpy(), *br.ball_query(q, t, 0.09, MAXN))


# ================================================================================================ ball_query()
def _ragged():
    t, q = nr.dense_cell()
    t2, q2 = nr.outside_grid()
    nt, nq = [900, 0, 333], [200, 30, 257]
    xyz = np.concatenate([t[:900, :3], t2[:333, :3]]).astype(F32)
    new = np.concatenate([q[:200], q[200:230], q2[:257]]).astype(F32)
    return xyz, nt, new, nq


def _check_batch(res, xyz, nt, new, nq, radius, nsample):
    """against one vg_ball_query_host call per batch element"""
    idx, empty = res
    assert idx.is_cuda and idx.dtype.is_floating_point is False and str(idx.dtype) == 'torch.int32' and str(empty.dtype) == 'torch.bool'
    idx, empty = idx.cpu().numpy(), empty.cpu().numpy()
    assert idx.shape == (len(new), nsample) and empty.shape == (len(new),)
    r = F32(radius)
    t0 = q0 = 0
    for n, m in zip(nt, nq):
        wi, wc = br.host(new[q0:q0 + m], xyz[t0:t0 + n].reshape(-1, 3), r * r, nsample)
        assert np.array_equal(idx[q0:q0 + m], wi) and np.array_equal(empty[q0:q0 + m], wc == 0), (t0, q0)
        t0, q0 = t0 + n, q0 + m


def test_ball_query_ragged_batch(cuda):
    """three batch elements, one of them without targets; the counts as lists and as tensors"""
    import torch
    from vilgod_amd import ball_query as bq
    xyz, nt, new, nq = _ragged()
    dx, dn = _dev(xyz, cuda), _dev(new, cuda)
    for radius, nsample in ((0.3, 100), (0.2, 1000), (0.5, 1)):
        _check_batch(bq.ball_query(radius, nsample, dx, nt, dn, nq), xyz, nt, new, nq, radius, nsample)
    res = bq.ball_query(0.3, 16, dx, torch.tensor(nt, dtype=torch.int32, device=cuda), dn, torch.tensor(nq, dtype=torch.int32, device=cuda))
    _check_batch(res, xyz, nt, new, nq, 0.3, 16)
    assert res[1][200:230].all() and not res[1][:200].all()
    with pytest.raises(ValueError, match='xyz_batch_cnt'):
        bq.ball_query(0.3, 16, dx, [900, 0, 332], dn, nq)
    with pytest.raises(ValueError, match='radius'):
        bq.ball_query(3.2, 16, dx, nt, dn, nq)
    with pytest.raises(ValueError, match='nsample'):
        bq.ball_query(0.3, bq.BALL_QUERY_MAX_NSAMPLE + 1, dx, nt, dn, nq)
    with pytest.raises(ValueError, match='new_xyz: float32'):
        bq.ball_query(0.3, 16, dx, nt, dn.double(), nq)


def test_ball_query_shared_model_and_growing_cache(cuda, model):
    import torch
    from vilgod_amd import ball_query as bq, knn as vk
    xyz, nt, new, nq = _ragged()
    dx, dn = _dev(xyz, cuda), _dev(new, cuda)
    # a caller's handle: used, not replaced, and no cached one is made for it
    before = dict(vk._handles)
    _check_batch(bq.ball_query(0.3, 50, dx, nt, dn, nq, model=model), xyz, nt, new, nq, 0.3, 50)
    assert vk._handles == before
    with pytest.raises(Exception):                                   # more targets than the caller's handle holds: an error, no silent second handle
        bq.ball_query(0.3, 4, torch.zeros((model.max_points + 1, 3), device=cuda), [model.max_points + 1], dn[:4], [4], model=model)
    # the cached handle (vilgod_amd.knn's, one per device): made on first use, kept, replaced by a larger one when more targets arrive
    old_min, vk._MIN_HANDLE_POINTS = vk._MIN_HANDLE_POINTS, 512
    try:
        vk._handles.clear()
        _check_batch(bq.ball_query(0.3, 8, dx[:300], [300], dn[:200], [200]), xyz[:300], [300], new[:200], [200], 0.3, 8)
        h0 = vk._handles[cuda.index]
        assert h0.max_points == 512
        _check_batch(bq.ball_query(0.3, 8, dx[:500], [500], dn[:200], [200]), xyz[:500], [500], new[:200], [200], 0.3, 8)
        assert vk._handles[cuda.index] is h0
        _check_batch(bq.ball_query(0.3, 8, dx, nt, dn, nq), xyz, nt, new, nq, 0.3, 8)
        h1 = vk._handles[cuda.index]
        assert h1 is not h0 and h1.max_points >= 900
        _check_batch(bq.ball_query(0.3, 8, dx[:300], [300], dn[:200], [200]), xyz[:300], [300], new[:200], [200], 0.3, 8)
        assert vk._handles[cuda.index] is h1
    finally:
        vk._MIN_HANDLE_POINTS = old_min
        vk._handles.clear()


def test_captured_graph_replays_with_new_queries(cuda, model):
    """grid + ball_query captured once: a replay reads the coordinates the query buffer holds then"""
    import torch
    t, q = nr.dense_cell()
    dt, dq = _dev(t, cuda), _dev(q, cuda)
    nsample, r2 = 100, F32(0.2)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):                              # warm-up outside the capture
        model.grid(dt)
        model.ball_query(dq, r2, nsample)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        model.grid(dt)
        idx, cnt = model.ball_query(dq, r2, nsample)
    moved = (q[::-1] + F32(0.07)).astype(F32)
    for qq in (q, moved):
        dq.copy_(torch.from_numpy(np.ascontiguousarray(qq)).to(cuda))
        graph.replay()
        torch.cuda.synchronize(cuda)
        want = br.ball_query(qq, t, r2, nsample)
        assert not br.same(idx.cpu().numpy(), cnt.cpu().numpy(), *want)
    assert br.same(*want, *br.ball_query(q, t, r2, nsample))


# ================================================================================================ the count wrappers
def test_count_neighbors_on_the_gpu(cuda, model):
    """numpy frames and CUDA tensors in, numpy out: the oracle's count matrix, the host path's, and the table's own count"""
    from oracle import neighbors_oracle as no
    from vilgod_amd import ball_query as bq
    rng = np.random.default_rng(3)
    base = rng.uniform(-2, 2, size=(700, 3)) * [1, 1, 0.2]
    frames = [(base[rng.random(700) < 0.8] + rng.normal(scale=0.05, size=(1, 3))).astype(F32) for _ in range(5)]
    want = no.count_neighbors(frames, seek=2, skip_frames=1)
    for buf in (frames, [_dev(f, cuda) for f in frames]):
        for kw in (dict(), dict(model=model)):
            got = bq.count_neighbors(buf, seek=2, skip_frames=1, **kw)
            assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(bq.count_neighbors(frames, seek=2, skip_frames=1, host=True), want)
    pts = frames[0]
    inter = bq.count_neighbors_inter_frame(pts, 0.2, 100)
    assert np.array_equal(inter, no.ball_count(pts, pts, nr.R2_INTER, 100)) and np.array_equal(inter, bq.count_neighbors_inter_frame(pts, 0.2, 100, host=True))
    # what the reference project computes from the index table is the same number
    idx, empty = bq.ball_query(0.2, 100, _dev(pts, cuda), [len(pts)], _dev(pts, cuda), [len(pts)])
    idx = idx.cpu().numpy()
    assert not empty.any().item() and np.array_equal(br.count_from_idx(idx), inter)
