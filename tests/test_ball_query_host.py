"""Ball query without a GPU: vg_ball_query_host (pcdet's loop as written, csrc/cluster_ball_query.inc) equals the dense numpy reference
of tests/ball_query_ref.py on every scene the device test runs -- every entry of idx and cnt, no tolerance --, the comparison rejects
synthesised faults, and the wrappers of vilgod_amd/ball_query.py check their arguments and count what the oracle counts.
"""
import numpy as np
import pytest

import ball_query_ref as br
import neighbors_ref as nr

F32 = np.float32


def _check(q, t, r2, nsample, d2=None):
    """host form == reference, and the count the reference project derives from the table == cnt"""
    wi, wc = br.from_d2(br.d2_matrix(q, t) if d2 is None else d2, r2, nsample)
    hi, hc = br.host(q, t, r2, nsample)
    msg = br.same(hi, hc, wi, wc)
    assert not msg, f'vg_ball_query_host vs reference, r2 {r2!r} nsample {nsample}: {msg}'
    full = wc > 0
    assert np.array_equal(br.count_from_idx(hi)[full], hc[full]) and (hi[~full] == 0).all()
    return wi, wc


# ================================================================================================ host form == reference
@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_threshold_pairs(offset):
    for r2 in nr.RADII:
        t, q = nr.threshold_pairs(offset, r2)
        d2 = br.d2_matrix(q, t)
        for nsample in (1, 3, 100):
            _check(q, t, r2, nsample, d2)


@pytest.mark.parametrize('offset', nr.OFFSETS)
def test_face_lattice(offset):
    t, q, _ = nr.face_lattice(offset)
    d2 = br.d2_matrix(q, t)
    for nsample in (1, 4, 100):
        _check(q, t, nr.R2_ENTROPY, nsample, d2)


def test_outside_grid():
    t, q = nr.outside_grid()
    d2 = br.d2_matrix(q, t)
    for r2 in nr.RADII:
        _check(q, t, r2, 16, d2)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_ties(order):
    """equidistant hits come out by row; at r2 == d2 exactly none is a hit"""
    t, q, info = nr.ties()
    t = t[br.orders(len(t))[order]]
    d2 = br.d2_matrix(q, t)
    above = np.nextafter(info['r2'], F32(np.inf))
    wi, wc = _check(q, t, above, 8, d2)
    assert wc[:info['n_ring']].min() >= 2 and wc.max() >= 6
    _, wc0 = _check(q, t, info['r2'], 8, d2)
    assert (wc0[:info['n_ring']] == 0).all()                  # (the coinciding queries behind them hit the target they sit on)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_dense_cell(order):
    """the hit counts per query lie below, around and above the kernel's buffer"""
    t, q = nr.dense_cell()
    assert len(t) == 3300 and len(q) == 512
    t = t[br.orders(len(t))[order]]
    d2 = br.d2_matrix(q, t)
    C = br.cand()
    spans = [((d2 < r2).sum(1).min(), (d2 < r2).sum(1).max()) for r2 in br.DENSE_R2]
    assert spans == [(0, 873), (0, 1901), (2153, 3003)] and spans[0][1] < C // 2 < spans[1][1] < C < spans[2][0]
    for r2 in br.DENSE_R2:
        for nsample in br.NSAMPLES:
            _check(q, t, r2, nsample, d2)


def test_built_scene_and_coincident_targets():
    C = br.cand()
    for hits in (C - 65, C - 64, C - 63, C - 1, C, C + 1, 2 * C, 2 * C + 1):
        for nsample in (1, 1023, 1024):
            t, q = br.built(hits, nsample)
            wi, wc = _check(q, t, nr.R2_ENTROPY, nsample)
            assert int((br.d2_matrix(q, t) < nr.R2_ENTROPY).sum()) == hits
            assert wc[0] == min(hits, nsample) and np.array_equal(wi[0, :wc[0]], np.arange(wc[0]))
    for inter in (False, True):
        t, q = br.coincident(inter, copies=3000)
        wi, wc = _check(q, t, nr.R2_ENTROPY, 1000)
        assert (wc == 1000).all() and np.array_equal(wi[5], np.arange(1000) * (2 if inter else 1))


def test_empty_degenerate_and_strides():
    t, q = nr.dense_cell()
    qq = br.nonfinite_rows(q)
    bad = ~np.isfinite(qq).all(1)
    wi, wc = _check(qq, t, nr.R2_ENTROPY, 9)
    assert (wc[bad] == 0).all() and (wi[bad] == 0).all() and (wc[~bad] > 0).any()
    tt = np.array(t[:400])
    tt[::7, 1] = np.nan; tt[3::7, 0] = np.inf                 # targets that are not points are never hits
    wi, wc = _check(q, tt, F32(0.2), 50)
    ok = np.isfinite(tt[:, :3]).all(1)
    assert ok[wi[wc > 0]].all() and (wc > 0).sum() > 100
    i0, c0 = br.host(q, np.zeros((0, 4), F32), 0.09, 5)       # no targets
    assert (i0 == 0).all() and (c0 == 0).all()
    i0, c0 = br.host(np.zeros((0, 3), F32), t, 0.09, 5)       # no queries
    assert i0.shape == (0, 5)
    want = br.ball_query(q[:100], t, 0.09, 7)
    for w in (3, 4, 7):                                       # floats per row: the columns behind z are not read
        qw = np.full((100, w), np.nan, F32); qw[:, :3] = q[:100]
        tw = np.full((len(t), w), np.nan, F32); tw[:, :3] = t[:, :3]
        assert not br.same(*br.host(qw, tw, 0.09, 7), *want)
    i1, c1 = br.host(q[:100], t, 0.09, 7, want_cnt=False)     # cnt NULL still writes idx
    assert not br.same(i1, None, *want) and (c1 == -7).all()
    big = br.host(q[:50], t, 400.0, 1024)                     # no reach limit on the host
    assert not br.same(*big, *br.ball_query(q[:50], t, 400.0, 1024)) and (big[1] == 1024).all()


def test_host_refusals():
    t, q = nr.dense_cell()
    from vilgod_amd.ball_query import BALL_QUERY_MAX_NSAMPLE as MAXN
    for kw in (dict(nsample=0), dict(nsample=-1), dict(nsample=MAXN + 1), dict(r2=0.0), dict(r2=-1.0), dict(r2=float('nan')), dict(qstride=2),
               dict(tstride=2)):
        a = dict(r2=0.09, nsample=4)
        a.update(kw)
        idx, cnt = br.host(q[:10], t, rc=1, **a)
        assert (idx == -7).all() and (cnt == -7).all(), kw


# ================================================================================================ the comparison rejects faults
def test_synthesised_faults_are_rejected():
    t, q = nr.dense_cell()
    d2 = br.d2_matrix(q, t)
    r2, nsample = F32(0.09), 64
    wi, wc = br.from_d2(d2, r2, nsample)
    assert not br.same(wi, wc, wi, wc)
    part = int(np.flatnonzero((wc >= 3) & (wc < nsample))[0])             # a row with hits and padding
    full = int(np.flatnonzero((d2 < r2).sum(1) > nsample)[0])             # a row the cap cuts
    # an unsorted row
    bad = wi.copy(); bad[part, [0, 1]] = bad[part, [1, 0]]
    assert br.same(bad, wc, wi, wc)
    bad = wi.copy(); bad[full, [10, 40]] = bad[full, [40, 10]]
    assert br.same(bad, wc, wi, wc)
    # the lowest row missing: the cap's window moved by one hit
    bad = wi.copy(); bad[full] = np.flatnonzero(d2[full] < r2)[1:nsample + 1]
    assert br.same(bad, wc, wi, wc)
    # padding with the last hit instead of the first
    bad = wi.copy(); bad[part, wc[part]:] = bad[part, wc[part] - 1]
    assert br.same(bad, wc, wi, wc)
    # a count that is off by one with the row intact
    bad = wc.copy(); bad[part] += 1
    assert br.same(wi, bad, wi, wc)
    # <= in place of < at a tie
    tt, tq, info = nr.ties()
    td2 = br.d2_matrix(tq, tt)
    want = br.from_d2(td2, info['r2'], 8)
    assert br.same(*br.from_d2(td2, info['r2'], 8, inclusive=True), *want)
    assert not br.same(*br.host(tq, tt, info['r2'], 8), *want)


# ================================================================================================ the wrappers
def test_ball_query_host_wrapper_ragged_batch():
    """three batch elements, one of them without targets and one without queries; rows count from the element's start"""
    from vilgod_amd import ball_query as bq
    t, q = nr.dense_cell()
    t2, q2 = nr.outside_grid()
    nt, nq = [900, 0, 333, 50], [200, 30, 257, 0]
    xyz = np.concatenate([t[:900, :3], t2[:333, :3], t[:50, :3]])
    new = np.concatenate([q[:200], q[200:230], q2[:257]])
    idx, empty = bq.ball_query_host(0.3, 100, xyz, nt, new, np.array(nq))
    assert idx.dtype == np.int32 and idx.shape == (487, 100) and empty.dtype == bool
    parts = [br.ball_query(q[:200], t[:900], nr.R2_ENTROPY, 100), br.ball_query(q[200:230], t[:0], nr.R2_ENTROPY, 100),
             br.ball_query(q2[:257], t2[:333], nr.R2_ENTROPY, 100)]
    assert np.array_equal(idx, np.concatenate([p[0] for p in parts])) and np.array_equal(empty, np.concatenate([p[1] for p in parts]) == 0)
    assert empty[200:230].all() and not empty[:200].all()


def test_wrappers_refuse_bad_arguments():
    import torch
    from vilgod_amd import ball_query as bq
    x, y = np.zeros((10, 3), F32), np.zeros((4, 3), F32)
    for fn in (bq.ball_query_host,):
        with pytest.raises(ValueError, match='nsample'):
            fn(0.3, 0, x, [10], y, [4])
        with pytest.raises(ValueError, match='nsample'):
            fn(0.3, bq.BALL_QUERY_MAX_NSAMPLE + 1, x, [10], y, [4])
        with pytest.raises(ValueError, match='radius'):
            fn(0.0, 4, x, [10], y, [4])
        with pytest.raises(ValueError, match='radius'):
            fn(float('nan'), 4, x, [10], y, [4])
        with pytest.raises(ValueError, match='xyz_batch_cnt'):
            fn(0.3, 4, x, [9], y, [4])
        with pytest.raises(ValueError, match='new_xyz_batch_cnt'):
            fn(0.3, 4, x, [10], y, [3, 2])
        with pytest.raises(ValueError, match='new_xyz_batch_cnt'):
            fn(0.3, 4, x, [10], y, [2, 2])
        with pytest.raises(ValueError, match='new_xyz'):
            fn(0.3, 4, x, [10], np.zeros((4, 2), F32), [4])
    assert bq.ball_query_host(5.0, 4, x, [10], y, [4])[0].shape == (4, 4)             # no radius limit on the host
    # the device form refuses before it touches a GPU
    tx, ty = torch.zeros((10, 3)), torch.zeros((4, 3))
    with pytest.raises(ValueError, match='xyz: a CUDA tensor'):
        bq.ball_query(0.3, 4, x, [10], ty, [4])
    with pytest.raises(ValueError, match='xyz: a CUDA tensor'):
        bq.ball_query(0.3, 4, tx, [10], ty, [4])
    with pytest.raises(ValueError, match='new_xyz: float32'):
        bq.ball_query(0.3, 4, tx, [10], ty.double(), [4])
    with pytest.raises(ValueError, match='xyz: .*dimensions'):
        bq.ball_query(0.3, 4, tx[None], [10], ty, [4])
    with pytest.raises(NotImplementedError, match='new_xyz'):
        bq.ball_query(0.3, 4, tx, [10], torch.zeros((4, 4)), [4])
    # radius: the grid reaches 8 cells; float32(3.2) squared is one float32 step above 10.24, so the last radius taken is the one below
    below = np.nextafter(F32(3.2), F32(0))
    assert bq._r2(below) == below * below and bq._r2(3.1) == F32(3.1) * F32(3.1)
    with pytest.raises(ValueError, match='radius'):
        bq._r2(3.2)
    with pytest.raises(ValueError, match='radius'):
        bq._r2(100.0)
    with pytest.raises(ValueError, match='radius'):
        bq._r2(-0.3)


def test_count_neighbors_equals_the_oracle():
    """the call shapes of pointcloud_utils.py:74-104 on numpy frames, kept off the GPU by host=True: the oracle's count matrix"""
    from oracle import neighbors_oracle as no
    from vilgod_amd import ball_query as bq
    rng = np.random.default_rng(3)
    base = rng.uniform(-2, 2, size=(700, 3)) * [1, 1, 0.2]
    frames = [(base[rng.random(700) < 0.8] + rng.normal(scale=0.05, size=(1, 3))).astype(F32) for _ in range(5)]
    frames = [np.c_[f, np.ones(len(f), F32)] for f in frames]             # a 4th column that is not read
    for seek, skip in ((0, 1), (2, 0), (4, 1)):
        got = bq.count_neighbors(frames, seek=seek, skip_frames=skip, host=True, some_other_keyword=1)
        want = no.count_neighbors(frames, seek=seek, skip_frames=skip)
        assert got.shape == want.shape == (len(frames[seek]), len(range(0, 5, skip + 1))) and got.dtype == np.int64
        assert np.array_equal(got, want) and got.max() > 3
    got = bq.count_neighbors(frames, seek=1, max_neighbor_point_dist=0.5, max_neighbor_points=5, host=True)
    assert np.array_equal(got, no.count_neighbors(frames, seek=1, max_neighbor_point_dist=0.5, max_neighbor_points=5)) and got.max() == 5
    pts = frames[0]
    inter = bq.count_neighbors_inter_frame(pts, 0.2, 100, host=True)
    assert np.array_equal(inter, no.ball_count(pts, pts, nr.R2_INTER, 100)) and inter.min() >= 1
