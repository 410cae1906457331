"""The fixed-radius neighbour queries (csrc/cluster_queries.inc: k_cl_ball_count, k_cl_nearest through vg_cluster_grid / _ball_count /
_nearest), the entropy score and the subsample keys (csrc/segment.hip: k_entropy_scores, k_subsample_keys) at their edges: pairs
exactly at the radius across cell faces, edges and corners, near the origin and 1 km from it; queries outside the grid and clamped
targets; equidistant targets in different cells; the cap; reach 8 and its refusal; block and stride shapes; the pairwise summation
at every frame count where it changes form.

CPU: the dense references of tests/neighbors_ref.py against the oracle (KD-tree candidates), and that every family really holds what
it is built for (a family that cannot fail proves nothing).  Every query of a family takes part in every comparison, whether or not
its construction hit the intended property.
GPU: the kernels through `HDBSCAN.grid / ball_count / nearest` and the C ABI against the dense references: counts, indices and the
float32 d2 bits are equal; entropy scores within 1e-12 of numpy and of a long-double sum.
"""
import functools

import numpy as np
import pytest

import neighbors_ref as nr
from oracle import neighbors_oracle as no

F32 = np.float32
BIG = 1 << 30
VG_ERR_ARG = 1
ALL_R2 = nr.RADII + (nr.R2_REACH1, nr.R2_REACH2)


# ------------------------------------------------------------------------------------------------------------ the cases
def _cases():
    """name -> (build() -> (targets, queries), radii, caps, gates)"""
    c = {}
    for off in nr.OFFSETS:
        for r2 in nr.RADII:
            c[f'threshold{list(off)}r2={float(r2):.4g}'] = (functools.partial(nr.threshold_pairs, off, r2), (r2,), (1000, 4), (r2,))
        for r2 in ALL_R2:
            c[f'lattice{list(off)}r2={float(r2):.4g}'] = (lambda off=off, r2=r2: nr.face_lattice(off, r2)[:2], (r2,), (1000, 2), (r2,))
    c['outside'] = (nr.outside_grid, ALL_R2, (1000, 2), (nr.R2_GATE, nr.R2_KNN, nr.R2_REACH2))
    for off in (nr.OFFSETS[0], nr.OFFSETS[3]):
        c[f'ties{list(off)}'] = (lambda off=off: nr.ties(off)[:2], (F32(0.0625), nr.R2_GATE, nr.R2_ENTROPY), (100, 3), (F32(0.0625), nr.R2_GATE))
    c['dense'] = (nr.dense_cell, nr.RADII, (1, 4, 100, 1000), (nr.R2_GATE,))
    c['reach'] = (nr.reach_limits, (nr.R2_REACH8, nr.R2_REACH1, nr.R2_REACH2), (1000, 100), (nr.R2_REACH8, nr.R2_REACH1))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def data(name):
    t, q = CASES[name][0]()
    assert t.dtype == F32 and q.dtype == F32 and len(t) <= 4096 and len(q) <= 4096
    return t, q


@functools.lru_cache(maxsize=None)
def want_counts(name, r2, inclusive=False):
    """uncapped dense counts, computed once per (case, radius) and shared by the CPU and GPU tests (read-only)"""
    t, q = data(name)
    c = nr.ball_count(q, t, r2, BIG, inclusive)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want_nearest(name, gate):
    t, q = data(name)
    return nr.nearest(q, t, gate)


# ------------------------------------------------------------------------------------------------------------ CPU: reference vs oracle
def test_d2_reference_matches_oracle_arithmetic():
    rng = np.random.default_rng(1)
    for off in nr.OFFSETS:
        q = (np.asarray(off) + rng.uniform(-3, 3, size=(20000, 3))).astype(F32)
        t = (q + rng.normal(scale=0.3, size=q.shape)).astype(F32)
        assert np.array_equal(nr.d2_f32(q, t), no.d2_f32(q, t))
    # one rounding, not two: 1 + (2^-24 + 2^-60) must round UP (the float64 sum drops the 2^-60 and lands on the float32 tie)
    a = np.array([1.0]); p = np.array([(2.0 ** -12 + 2.0 ** -36) * 2.0 ** -12])
    assert nr._round_sum(p, a)[0] == np.nextafter(F32(1), F32(2))
    assert nr._round_sum(np.array([2.0 ** -24]), a)[0] == F32(1)                # the exact tie goes to even


@pytest.mark.parametrize('name', list(CASES))
def test_dense_reference_matches_oracle(name):
    """... which also checks the oracle's enlarged KD-tree radius 1 km from the origin."""
    t, q = data(name)
    _, radii, caps, gates = CASES[name]
    for r2 in radii:
        full = want_counts(name, r2)
        for cap in (BIG, caps[-1]):
            assert np.array_equal(np.minimum(full, cap), no.ball_count(q, t, r2, cap)), (name, r2, cap)
    for g in gates:
        idx, d2 = want_nearest(name, g)
        oi, od = no.nearest(q, t, g)
        assert np.array_equal(idx, oi) and np.array_equal(d2.view(np.int32), od.view(np.int32)), (name, g)


# ------------------------------------------------------------------------------------------------------------ CPU: the families hold what they claim
@pytest.mark.parametrize('off', nr.OFFSETS)
def test_threshold_family_sits_at_the_radius(off):
    for r2 in nr.RADII:
        name = f'threshold{list(off)}r2={float(r2):.4g}'
        t, q = data(name)
        assert len(t) == 600 and np.abs(t[:, :3] - np.asarray(off, F32)).max() <= 6.001
        qi, ti, st = nr.threshold_pairs_of(q, t, r2)
        assert len(qi) >= 200 and (st < 0).sum() >= 50 and (st > 0).sum() >= 50, (off, r2, len(qi))
        assert (st == 0).sum() >= 50, (off, r2, (st == 0).sum())
        # '<' and '<=' differ exactly at those pairs, so a kernel with the wrong comparison cannot pass
        strict, incl = want_counts(name, r2), want_counts(name, r2, True)
        assert (incl - strict).sum() == (st == 0).sum() and (incl != strict).sum() >= 50
        # every direction and both senses are there among the pairs AT the radius
        d = (q[qi[st == 0]] - t[ti[st == 0], :3]).astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        for u in nr.DIRS:
            for s in (1.0, -1.0):
                assert ((d @ nr._unit(u, s)) > 0.998).sum() >= 3, (off, r2, u, s)
        # the exact (float64) distance of these pairs is within the float32 rounding of r2: they ARE at the threshold
        ex = nr.d2_exact(q[qi], t[ti, :3])
        assert np.all(np.abs(ex - float(r2)) <= 8 * float(np.spacing(r2)))


@pytest.mark.parametrize('off', nr.OFFSETS)
def test_lattice_family_straddles_faces_edges_and_corners(off):
    for r2 in ALL_R2:
        t, q, A = nr.face_lattice(off, r2)
        o = nr.grid_origin(t)
        assert np.array_equal(o, A), (o, A)                                    # the two anchors fix the origin
        # the targets are ON the computed faces, one float32 step below, or one above
        rel = t[2:, :3].astype(np.float64)
        face = (A + np.round((rel - A) / nr.CELL) * nr.CELL).astype(F32)
        for s, lim in ((-1, F32(-np.inf)), (1, F32(np.inf))):
            assert ((t[2:, :3] == np.nextafter(face, lim)).sum(0) >= 60).all()
        assert ((t[2:, :3] == face).sum(0) >= 60).all()
        qi, ti, st = nr.threshold_pairs_of(q, t, r2)
        n_axes = (nr.cell_of(q[qi], o) != nr.cell_of(t[ti], o)).sum(1)
        assert ((n_axes == 1).sum() >= 100 and (n_axes == 2).sum() >= 100 and (n_axes == 3).sum() >= 100), (off, r2, np.bincount(n_axes))
        if r2 in (nr.R2_REACH1, nr.R2_REACH2):                                  # ... `reach` cells away: the farthest cell the kernel looks at
            reach = int(np.ceil(np.sqrt(float(r2)) / nr.CELL))
            far = np.abs(nr.cell_of(q[qi], o) - nr.cell_of(t[ti], o)).max(1)
            assert (far == reach).sum() >= 100
        inside = st < 0
        assert inside.sum() >= 100 and (~inside).sum() >= 100                   # just inside and just outside (or at) the radius


def test_outside_family_leaves_the_grid_on_every_side():
    t, q = nr.outside_grid()
    o = nr.grid_origin(t)
    ct, cq = nr.cell_unclamped(t, o), nr.cell_unclamped(q, o)
    for a in range(3):
        assert t[:, a].max() - t[:, a].min() > nr.EXT[a]
        assert (ct[:, a] >= nr.NB[a]).sum() >= 20                               # targets beyond the last cell: clamped
        assert (cq[:, a] < 0).sum() >= 20 and (cq[:, a] >= nr.NB[a]).sum() >= 20
        far = nr.cell_unclamped(q, o)[:, a] >= nr.NB[a] + 100                   # ~50 m beyond
        assert far.sum() >= 20 and (cq[:, a] < -100).sum() >= 20
        # a query in the last regular cell with a clamped neighbour in the border cell, on both sides of r2 = 0.2
        idx, d2 = nr.nearest(q, t, nr.R2_REACH2)
        pair = (cq[:, a] == nr.NB[a] - 2) & (idx >= 0) & (ct[np.maximum(idx, 0), a] >= nr.NB[a])
        assert (pair & (d2 < nr.R2_GATE)).sum() >= 5 and (pair & (d2 > nr.R2_GATE)).sum() >= 5, a
    # queries beyond the grid WITH neighbours there (both clamped into a border cell): the counts are not all zero out there
    outq = ((cq < 0) | (cq >= np.array(nr.NB))).any(1)
    assert (want_counts('outside', nr.R2_ENTROPY)[outq] > 0).sum() >= 100
    assert (nr.cell_of(q, o) == nr.cell_of(t[np.maximum(nr.nearest(q, t, nr.R2_GATE)[0], 0)], o)).all(1)[outq].sum() >= 100


@pytest.mark.parametrize('off', (nr.OFFSETS[0], nr.OFFSETS[3]))
def test_ties_family_is_exactly_equidistant_across_cells(off):
    t, q, info = nr.ties(off)
    o = nr.grid_origin(t)
    assert np.array_equal(o, info['A'])
    n = info['n_ring']
    d2 = nr.d2_f32(q[:n, None, :], t[None, :, :3])
    ring = d2 == info['r2']
    k = ring.sum(1)
    assert k.min() >= 2 and set(np.unique(k)) >= {2, 3, 4, 5, 6} and (d2 < info['r2']).sum() == 0
    cq = nr.cell_of(q[:n], o)
    first_row = ring.argmax(1)
    last_visited = np.array([0, 0, 1]); first_visited = np.array([0, 0, -1])
    delta = nr.cell_of(t[first_row], o) - cq
    for i in range(n):
        cells = {tuple(c) for c in nr.cell_of(t[ring[i]], o) - cq[i]}
        assert (0, 0, 0) in cells and len(cells) >= 2
    assert (np.abs(delta).sum(1) > 0).sum() >= 100                              # the lowest row lies outside the own cell
    assert (delta == first_visited).all(1).sum() >= 40 and (delta == last_visited).all(1).sum() >= 40 and (delta == 0).all(1).sum() >= 40
    # duplicates at other rows, queries ON a target
    uniq, cnt = np.unique(t[:, :3], axis=0, return_counts=True)
    assert (cnt >= 2).sum() >= 60
    zero = nr.d2_f32(q[n:, None, :], t[None, :, :3]) == 0
    assert zero.any(1).all() and (zero.sum(1) >= 2).sum() >= 30
    # '<' against '<=' at the ring
    assert np.array_equal(nr.ball_count(q[:n], t, info['r2'], BIG, True) - nr.ball_count(q[:n], t, info['r2'], BIG), k)


def test_dense_and_reach_families():
    t, q = nr.dense_cell()
    assert len(t) >= 3000
    for cap in (1, 4, 100, 1000):                                               # queries on both sides of every cap
        full = np.concatenate([want_counts('dense', r2) for r2 in nr.RADII])
        assert (full > cap).sum() >= 20 and (full < cap).sum() >= 20, cap
    t, q = nr.reach_limits()
    assert len(q) == 64
    for r2, reach in ((nr.R2_REACH8, 8), (nr.R2_REACH1, 1), (nr.R2_REACH2, 2)):
        assert int(np.ceil(np.sqrt(np.float64(r2)) / nr.CELL)) == reach
    assert int(np.ceil(np.sqrt(np.float64(np.nextafter(nr.R2_REACH8, F32(11)))) / nr.CELL)) == 9
    # neighbours really lie 8 cells away, so a host that looked at 7 would lose them
    o = nr.grid_origin(t)
    d2 = nr.d2_f32(q[:, None, :], t[None, :, :3])
    i, j = np.nonzero(d2 < nr.R2_REACH8)
    assert (np.abs(nr.cell_of(q[i], o) - nr.cell_of(t[j], o)).max(1) == 8).sum() >= 50


# ------------------------------------------------------------------------------------------------------------ CPU: entropy and keys
FRAMES = (2, 7, 8, 9, 15, 16, 17, 24, 127, 128)
NQS = (1, 127, 128, 129, 1000)
SEEDS = (0, 1, 1 << 63, (1 << 64) - 1)
TAGS = (0, 198, (1 << 32) - 1, 1 << 32)


def _seeks(n):
    return (-1, 0, n // 2, n - 1)


def _with_seek(c, seek):
    c = c.astype(np.int64)
    if seek >= 0:
        c[:, seek] -= 1
    return c


def _entropy_err(got, want):
    """largest |got - want| where want is finite; NaN must meet NaN"""
    want = np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    return float(np.abs(got[~nan] - want[~nan]).max()) if (~nan).any() else 0.0


def test_entropy_count_matrices_hold_the_special_rows():
    for n in FRAMES:
        c = nr.count_matrices(n, 128)
        assert c.dtype == np.int32 and c.min() == 0 and c.max() == 1000
        assert (c == 0).all(1).any() and (c == 1000).all(1).any() and ((c > 0).sum(1) == 1).sum() >= 3
        assert ((c > 0).sum(1) == 1)[(c[:, -1] > 0)].any()                      # one non-zero frame: the last one


def test_numpy_oracle_agrees_with_long_double_reference():
    worst = 0.0
    for n in FRAMES:
        c = nr.count_matrices(n, 1000)
        for seek in _seeks(n):
            with np.errstate(invalid='ignore', divide='ignore'):
                H = no.compute_ephe_score(_with_seek(c, seek))
            worst = max(worst, _entropy_err(H, nr.ephe_score(c, seek)))
    print(f'\nnumpy oracle against the long-double sum: largest error {worst / 1e-12:.2e} of the 1e-12 bound')
    assert worst <= 1e-12


def test_key_reference_matches_oracle():
    for seed in SEEDS:
        for tag in TAGS:
            for n in (1, 255, 256, 257):
                assert np.array_equal(nr.subsample_keys(seed, tag, n), no.subsample_keys(seed, tag, n)), (seed, tag, n)
    assert np.array_equal(nr.subsample_keys(7, 198, 65537)[-300:], no.subsample_keys(7, 198, 65537)[-300:])
    assert np.array_equal(nr.subsample_keys(5, 1 << 32, 300), nr.subsample_keys(5, 0, 300))          # tag << 32 wraps
    assert nr.subsample_keys((1 << 64) - 1, (1 << 32) - 1, 4096).min() >= 0


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def model(cuda):
    from vilgod_amd.hdbscan import HDBSCAN
    return HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15, max_points=8192)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _check_case(model, cuda, name):
    t, q = data(name)
    _, radii, caps, gates = CASES[name]
    dt, dq = _dev(t, cuda), _dev(q, cuda)
    model.grid(dt)
    for r2 in radii:
        full = want_counts(name, r2)
        for cap in caps:
            got = model.ball_count(dq, r2, cap).cpu().numpy()
            assert np.array_equal(got, np.minimum(full, cap)), f'{name} r2 {r2!r}\n' + nr.explain_counts(q, t, r2, cap, got)
            assert np.array_equal(model.ball_count(dq, r2, cap).cpu().numpy(), got), (name, r2, cap, 'second run differs')
    for g in gates:
        widx, wd2 = want_nearest(name, g)
        idx, d2 = (x.cpu().numpy() for x in model.nearest(dq, g))
        assert np.array_equal(idx, widx) and np.array_equal(d2.view(np.int32), wd2.view(np.int32)), \
            f'{name} gate {g!r}\n' + nr.explain_nearest(q, t, g, idx, d2)
        idx2, d22 = (x.cpu().numpy() for x in model.nearest(dq, g))
        assert np.array_equal(idx2, idx) and np.array_equal(d22.view(np.int32), d2.view(np.int32)), (name, g, 'second run differs')


@pytest.mark.gpu
@pytest.mark.parametrize('off', nr.OFFSETS)
def test_pairs_at_the_radius_gpu(cuda, model, off):
    for r2 in nr.RADII:
        _check_case(model, cuda, f'threshold{list(off)}r2={float(r2):.4g}')


@pytest.mark.gpu
@pytest.mark.parametrize('off', nr.OFFSETS)
def test_pairs_across_faces_edges_corners_gpu(cuda, model, off):
    for r2 in ALL_R2:
        _check_case(model, cuda, f'lattice{list(off)}r2={float(r2):.4g}')


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if not n.startswith(('threshold', 'lattice'))])
def test_outside_ties_cap_reach_gpu(cuda, model, name):
    _check_case(model, cuda, name)


@pytest.mark.gpu
def test_reach_refusals_and_bad_arguments_gpu(cuda, model):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    t, q = nr.reach_limits()
    dt, dq = _dev(t, cuda), _dev(q, cuda)
    model.grid(dt)
    h = model._h
    cnt = torch.full((len(q),), -7, dtype=torch.int32, device=cuda)
    idx = torch.full((len(q),), -7, dtype=torch.int32, device=cuda)
    d2 = torch.full((len(q),), -7.0, dtype=torch.float32, device=cuda)
    ok8, over = float(nr.R2_REACH8), float(np.nextafter(nr.R2_REACH8, F32(11)))

    def count(nq=len(q), stride=3, r2=ok8, cap=10):
        return lib.vg_cluster_ball_count(h, ptr(dq), nq, stride, r2, cap, ptr(cnt), stream_ptr())

    def near(nq=len(q), stride=3, r2=ok8):
        return lib.vg_cluster_nearest(h, ptr(dq), nq, stride, r2, ptr(idx), ptr(d2), stream_ptr())

    # reach 9 (the next float32 above 10.24), r2 <= 0 (and NaN), a stride below 3, a negative cap, nq < 0: refused, nothing written
    assert count(r2=over) == VG_ERR_ARG and near(r2=over) == VG_ERR_ARG
    for bad in (0.0, -1.0, float('nan')):
        assert count(r2=bad) == VG_ERR_ARG and near(r2=bad) == VG_ERR_ARG
    assert count(stride=2) == VG_ERR_ARG and near(stride=2) == VG_ERR_ARG
    assert count(cap=-1) == VG_ERR_ARG and count(nq=-1) == VG_ERR_ARG and near(nq=-1) == VG_ERR_ARG
    assert lib.vg_cluster_grid(h, ptr(dt), len(t), 2, stream_ptr()) == VG_ERR_ARG
    assert lib.vg_cluster_grid(h, ptr(dt), -1, 4, stream_ptr()) == VG_ERR_ARG
    torch.cuda.synchronize()
    assert int((cnt != -7).sum()) == 0 and int((idx != -7).sum()) == 0 and int((d2 != -7.0).sum()) == 0
    # ... and the refused grid calls left the grid alone: reach 8 itself is accepted
    assert count(cap=1000) == 0 and near() == 0
    assert np.array_equal(cnt.cpu().numpy(), np.minimum(want_counts('reach', nr.R2_REACH8), 1000))
    assert np.array_equal(idx.cpu().numpy(), want_nearest('reach', nr.R2_REACH8)[0])
    # cap 0 is a valid cap
    assert int(model.ball_count(dq, nr.R2_ENTROPY, 0).abs().sum()) == 0


@pytest.mark.gpu
def test_shapes_strides_empty_sets_and_rebuild_gpu(cuda, model):
    import torch
    name = f'threshold{list(nr.OFFSETS[1])}r2={float(nr.R2_ENTROPY):.4g}'
    t, q = data(name)
    r2 = nr.R2_ENTROPY
    full, (widx, wd2) = want_counts(name, r2), want_nearest(name, r2)
    dt = _dev(t, cuda)
    model.grid(dt)
    rng = np.random.default_rng(3)
    for nq in (1, 255, 256, 257):
        for stride in (3, 4, 5):
            qq = np.full((nq, stride), 1e9, F32)                                   # columns past z must not be read as coordinates
            qq[:, :3] = q[1000:1000 + nq]
            dq = _dev(qq, cuda)
            tail = torch.full((nq + 64,), -7, dtype=torch.int32, device=cuda)      # rows past nq must not be written
            got = model.ball_count(dq, r2, 1000, out=tail[:nq]).cpu().numpy()
            assert np.array_equal(got, full[1000:1000 + nq]), f'nq {nq} stride {stride}\n' + nr.explain_counts(qq, t, r2, 1000, got)
            assert int((tail[nq:] != -7).sum()) == 0
            idx, d2 = (x.cpu().numpy() for x in model.nearest(dq, r2))
            assert np.array_equal(idx, widx[1000:1000 + nq]) and np.array_equal(d2, wd2[1000:1000 + nq]), (nq, stride)
    # target stride 3 and 5 give the same grid as stride 4
    dq = _dev(q, cuda)
    for stride in (3, 5):
        tt = np.full((len(t), stride), 1e9, F32)
        tt[:, :3] = t[:, :3]
        model.grid(_dev(tt, cuda))
        assert np.array_equal(model.ball_count(dq, r2, 1000).cpu().numpy(), full), stride
    # empty query set; empty target set: zeros and (-1, +inf)
    assert model.ball_count(dq[:0], r2, 10).numel() == 0 and model.nearest(dq[:0], r2)[0].numel() == 0
    model.grid(dt[:0])
    assert int(model.ball_count(dq, r2, 10).abs().sum()) == 0
    idx, d2 = model.nearest(dq, r2)
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all())
    # a second target set on the same handle: fewer points, the same place -- nothing of the first grid may remain
    model.grid(dt)
    t2 = t[rng.permutation(len(t))[:37]].copy()
    t2[:, :3] += F32(0.05)
    model.grid(_dev(t2, cuda))
    got = model.ball_count(dq, nr.R2_GATE, 1000).cpu().numpy()
    assert np.array_equal(got, nr.ball_count(q, t2, nr.R2_GATE, 1000)), nr.explain_counts(q, t2, nr.R2_GATE, 1000, got)
    idx, d2 = (x.cpu().numpy() for x in model.nearest(dq, nr.R2_GATE))
    wi, wd = nr.nearest(q, t2, nr.R2_GATE)
    assert np.array_equal(idx, wi) and np.array_equal(d2, wd) and idx.max() < 37
    model.grid(dt)                                                              # ... and back
    assert np.array_equal(model.ball_count(dq, r2, 1000).cpu().numpy(), full)


class _MadeUpTree:
    """An HDBSCAN handle whose clustering is replaced by made-up labels: TwoFrameClusterer.labels then runs its own label transfer
    (grid over the clustering input, nearest within the gate, gather) on the real kernels."""

    def __init__(self, model, labels, probs, hierarchy, cuda):
        self._m, self._lab, self._prob, self.hierarchy, self._cuda = model, labels, probs, hierarchy, cuda

    def __getattr__(self, k):
        return getattr(self._m, k)

    def mst(self, seq, dim=3):
        import torch
        e = torch.empty(0, device=self._cuda)
        return e, e, e

    def tree(self, lo, hi, w2, n):
        return self._lab.astype(np.int32), self._prob, 10

    def tree_device(self, lo, hi, w2, n):
        return _dev(self._lab.astype(np.int32), self._cuda), _dev(self._prob, self._cuda), None


@pytest.mark.gpu
@pytest.mark.parametrize('hierarchy', ['host', 'device'])
def test_label_transfer_outside_the_grid_gpu(cuda, model, hierarchy):
    from vilgod_amd.entropy import TwoFrameClusterer
    t, q = nr.outside_grid()
    rng = np.random.default_rng(5)
    labels, probs = rng.integers(0, 10, len(t)), rng.random(len(t))
    seq = np.c_[t, np.zeros(len(t), F32)].astype(F32)                            # [x, y, z, entropy, 0.1 * frame]
    two = TwoFrameClusterer(_MadeUpTree(model, labels, probs, hierarchy, cuda), n_frames=2, seed=0)
    dseq = _dev(seq, cuda)
    two.cluster_input = lambda fnr, X_list, ent_list: dseq
    dq = _dev(np.c_[q, np.ones(len(q), F32)].astype(F32), cuda)
    lab, prob = two.labels(1, [dq, dq], [None, None])
    wl, wp = no.knn_labels(q, t[:, :3], labels, probs)
    assert np.array_equal(lab, wl) and np.array_equal(prob, wp)
    assert F32(two.gate) == nr.R2_KNN
    beyond = want_nearest('outside', nr.R2_KNN)[0] < 0
    assert np.array_equal(lab == -1, beyond) and beyond.sum() >= 100 and (~beyond).sum() >= 100


@pytest.mark.gpu
@pytest.mark.parametrize('n_frames', FRAMES)
def test_entropy_scores_summation_gpu(cuda, n_frames):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    worst_np, worst_ld = 0.0, 0.0
    for nq in NQS:
        c = nr.count_matrices(n_frames, nq)
        for seek in _seeks(n_frames):
            cc = c.copy()
            if seek >= 0:
                cc[:, seek] += (np.arange(nq) % 3 != 0)               # the seek frame counts the query itself; every third row goes negative
            dc = _dev(cc.T, cuda)
            H = torch.full((nq + 32,), -7.0, dtype=torch.float64, device=cuda)
            assert lib.vg_entropy_scores(ptr(dc), n_frames, nq, seek, ptr(H), stream_ptr()) == 0
            got = H.cpu().numpy()
            assert np.all(got[nq:] == -7.0)
            with np.errstate(invalid='ignore', divide='ignore'):
                want = no.compute_ephe_score(_with_seek(cc, seek))
            assert np.allclose(got[:nq], want, rtol=0, atol=1e-12, equal_nan=True), (n_frames, nq, seek)
            worst_np = max(worst_np, _entropy_err(got[:nq], want))
            worst_ld = max(worst_ld, _entropy_err(got[:nq], nr.ephe_score(cc, seek)))
    print(f'\nentropy n_frames {n_frames}: largest error {worst_np / 1e-12:.2e} of the 1e-12 bound against numpy, '
          f'{worst_ld / 1e-12:.2e} against the long-double sum')
    assert worst_ld <= 1e-12


@pytest.mark.gpu
def test_entropy_scores_refusals_gpu(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    dc = torch.ones((129, 16), dtype=torch.int32, device=cuda)
    H = torch.full((16,), -7.0, dtype=torch.float64, device=cuda)
    for n in (1, 129, 0, -1):
        assert lib.vg_entropy_scores(ptr(dc), n, 16, -1, ptr(H), stream_ptr()) == VG_ERR_ARG
    assert lib.vg_entropy_scores(ptr(dc), 8, -1, -1, ptr(H), stream_ptr()) == VG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((H == -7.0).all())


@pytest.mark.gpu
def test_subsample_keys_wraps_and_blocks_gpu(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    for n in (1, 255, 256, 257, 65537):
        k = torch.full((n + 16,), -7, dtype=torch.int64, device=cuda)
        for seed in SEEDS:
            for tag in TAGS:
                assert lib.vg_subsample_keys(seed, tag, n, ptr(k), stream_ptr()) == 0
                got = k.cpu().numpy()
                assert np.array_equal(got[:n], nr.subsample_keys(seed, tag, n)), (seed, tag, n)
                assert got[:n].min() >= 0 and np.all(got[n:] == -7)
    assert lib.vg_subsample_keys(0, 0, -1, ptr(k), stream_ptr()) == VG_ERR_ARG
