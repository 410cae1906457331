"""The Boruvka MST of csrc/cluster_mst.inc (geometry: cluster_geom.inc) at its edges: the geometry its walks prune with (CPU, through vg_cluster_geom_probe, on the
shipped source) and scenes aimed at each pruning rule (GPU, exact against the oracle).

CPU part.  The walk skips a node when its box distance exceeds the best candidate, so the box distance has to be a LOWER BOUND of the
float64 pair distance to every point the node holds, and the shell radius of the cooperative searches a lower bound for every point
outside the 27 nodes of the shell.  Both are checked for float32 coordinates 0, 1 and 2 steps from every face, for many origins, for
points clamped into border cells, at all seven levels.  The formulas used before cells were assigned by the computed faces fail this
(tests/mst_ref.py keeps them as `parent_*`; `test_parent_formulas_were_no_lower_bound` shows the failure on the lattice scenes).

GPU part.  Every scene is compared like tests/test_cluster.py::test_hip_core_mst_labels_equal_oracle: core distances, sorted weights,
edge set, labels and probabilities in both hierarchy modes, bit for bit, with min_samples = 15 and 1 and in three point orders (ids
break ties).
"""
import numpy as np
import pytest

import mst_ref as mr
from oracle import hdbscan_oracle as ho

F32 = np.float32
NB = mr.NB


# ================================================================================================ CPU: geometry through the probe
def _anchor_bbox(anchor):
    a = np.asarray(anchor, F32)
    return a - F32([30, 30, 3]), a + F32([30, 30, 3])


def _random_bboxes(count=400, seed=7):
    """|coordinate| <= 1200 m, spans from 0.5 m to beyond the grid's extent (204.8 m / 25.6 m)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        span = np.exp(rng.uniform(np.log(0.5), np.log([400.0, 400.0, 60.0])))
        lo = rng.uniform(-1200.0, 1200.0 - span)
        out.append((lo.astype(F32), (lo + span).astype(F32)))
    return out


def _origins():
    """[(name, origin [3] float64, full query set?)]: anchors, lattice scenes and 400 random boxes.  EVERY face of every axis at every
    origin; the random boxes get the shorter query list of `_pairs` (the suite runs on every change)."""
    out = []
    for a in mr.ANCHORS:
        out.append((f'anchor{a}', mr.probe(points=np.zeros((1, 3), F32), bbox=_anchor_bbox(a))['origin'], True))
    for name in mr.LATTICE_NAMES:
        X, _ = mr.lattice_scene(name)
        out.append((name, mr.probe(points=X[:1], bbox=mr.bbox_of(X))['origin'], True))
    for i, bb in enumerate(_random_bboxes()):
        out.append((f'random{i}', mr.probe(points=np.zeros((1, 3), F32), bbox=bb)['origin'], False))
    return out


def _axis_values(origin, axis):
    """float32 values 0, +-1, +-2 steps from EVERY face of the axis, and beyond the grid on both sides"""
    return np.unique(np.concatenate([mr.face_values(origin, axis), mr.outside_values(origin, axis)]))


def _pairs(origin, full):
    """(points [m,3], queries [m,3]) float32.  Along each axis: points 0, +-1, +-2 float32 steps from the faces and beyond the grid on
    both sides; queries the 5 neighbouring values on either side (inside, on and just outside the node), 0.3 .. 60 m away on either side
    and beyond the grid.  The other two coordinates are equal (the axis distance is the whole distance: the sharpest case) or sit a step
    from a face themselves.  `full` = False (the 400 random origins): the 3 neighbouring values on either side, 0.3 and 7 m, beyond the
    grid, equal other coordinates only -- the same faces, the queries next to them, a fifth of the pairs."""
    P, Q = [], []
    for a in range(3):
        v = _axis_values(origin, a)
        m = len(v)
        j = np.arange(m)
        reach = 5 if full else 3
        qs = [v[np.clip(j + s, 0, m - 1)] for s in range(-reach, reach + 1)]
        qs += [(v.astype(np.float64) + d).astype(F32) for d in ((-60.0, -7.0, -1.1, -0.3, 0.3, 1.1, 7.0, 60.0) if full else (-7.0, -0.3, 0.3, 7.0))]
        qs += [np.full(m, o, F32) for o in mr.outside_values(origin, a)]
        q = np.stack(qs, 1)                                                       # [m, nq]
        p = np.repeat(v[:, None], q.shape[1], 1)
        b, c = (a + 1) % 3, (a + 2) % 3
        for variant in range(2 if full else 1):
            pp = np.zeros(p.shape + (3,), F32)
            qq = np.zeros(p.shape + (3,), F32)
            pp[..., a], qq[..., a] = p, q
            if variant == 0:
                pp[..., b] = qq[..., b] = F32(origin[b] + 100.5 * mr.CELL)
                pp[..., c] = qq[..., c] = F32(origin[c] + 30.5 * mr.CELL)
            else:
                fb = F32(origin[b] + 200 * mr.CELL)
                pp[..., b], qq[..., b] = fb, mr.steps(fb, -1)
                pp[..., c], qq[..., c] = F32(origin[c] + 30.5 * mr.CELL), F32(origin[c] + 30.5 * mr.CELL + 0.3)
            P.append(pp.reshape(-1, 3))
            Q.append(qq.reshape(-1, 3))
    return np.concatenate(P), np.concatenate(Q)


def test_box_distance_is_a_lower_bound_at_every_level():
    """box_d2(q, node_l(p)) <= d2(q, p) for l = 0 .. 6."""
    total, bad = 0, []
    for name, origin, all_faces in _origins():
        P, Q = _pairs(origin, all_faces)
        r = mr.probe(points=P, queries=Q, origin=origin, want_code=False)
        d2 = mr.d2_f64(Q, P)
        v = r['box_d2'] > d2[:, None]
        total += v.size
        for i, l in zip(*np.nonzero(v)):
            bad.append((name, origin.tolist(), P[i].tolist(), Q[i].tolist(), int(l), float(r['box_d2'][i, l] - d2[i])))
    print(f'{total} point/query/level triples')
    assert total > 3_000_000
    assert not bad, (len(bad), bad[:5])


def test_parent_formulas_were_no_lower_bound():
    """The demonstration: the formulas of the parent commit (mst_ref.parent_box_d2) on the same pairs, at the origins of the lattice
    scenes that were chosen for it.  They must FAIL the property there -- otherwise the scenes are not aimed at anything."""
    for name in mr.LATTICE_NAMES:
        X, axes = mr.lattice_scene(name)
        if not axes:
            continue
        origin = mr.parent_origin(X)
        P, Q = _pairs(origin, True)
        d2 = mr.d2_f64(Q, P)
        n_bad = sum(int((mr.parent_box_d2(origin, Q, P, l) > d2).sum()) for l in range(mr.LMAX + 1))
        print(f'{name}: {n_bad} violations of the earlier formulas')
        assert n_bad > 0, name


def test_cells_agree_with_the_computed_faces():
    """Containment, stated directly: the faces are o + i * 0.4 as computed in float64; a point of cell c lies in [face(c), face(c + 1))
    unless it was clamped (cell 0 holds everything below, the last cell everything above)."""
    for name, origin, all_faces in _origins()[:24]:
        for a in range(3):
            v = _axis_values(origin, a)
            P = np.zeros((len(v), 3), F32) + origin.astype(F32)
            P[:, a] = v
            c = mr.probe(points=P, origin=origin)['cell'][:, a].astype(np.int64)
            lo, hi = origin[a] + c.astype(np.float64) * mr.CELL, origin[a] + (c + 1).astype(np.float64) * mr.CELL
            v64 = v.astype(np.float64)
            assert (((v64 >= lo) | (c == 0)) & ((v64 < hi) | (c == NB[a] - 1))).all(), (name, a)
            assert (np.diff(c) >= 0).all() and c.min() == 0 and c.max() == NB[a] - 1          # monotone, every border cell reached


def test_block_radius_is_a_lower_bound_outside_the_shell():
    """cl_block_radius2(q, level l): every point whose level-l node is not one of the 27 nodes around q's is at least that far.
    DEVIATION from "every face": all query x point pairs of an axis are formed here, so the values come from a list of faces (the grid's
    borders, the faces around the 2^l-aligned ones of every level, the middle) at the 13 all-query origins and 40 of the random ones.
    The radius is computed from the same faces o + i * s as the boxes, which the box test covers at every face of every origin."""
    checked = 0
    for name, origin, _ in [o for o in _origins() if o[2]] + _origins()[-40:]:
        for a in range(3):
            n = NB[a]
            faces = np.unique(np.clip(np.concatenate([np.arange(0, 6), [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65], np.arange(n // 2 - 2, n // 2 + 3),
                                                      np.arange(n - 5, n + 1)]), 0, n))
            v = np.unique(np.concatenate([mr.face_values(origin, a, faces), mr.outside_values(origin, a)]))
            m = len(v)
            for variant in range(2):
                base = np.zeros((m, 3), F32)
                b, c = (a + 1) % 3, (a + 2) % 3
                base[:, b] = F32(origin[b] + 100.5 * mr.CELL) if variant == 0 else mr.steps(F32(origin[b] + 96 * mr.CELL), 1)
                base[:, c] = F32(origin[c] + 30.5 * mr.CELL) if variant == 0 else mr.steps(F32(origin[c] + 32 * mr.CELL), -1)
                base[:, a] = v
                r = mr.probe(points=base, queries=base, origin=origin, want_code=False)
                cell = r['cell'][:, a].astype(np.int64)
                d2 = mr.d2_f64(base[:, None, :], base[None, :, :])                         # [query, point]
                for l in range(mr.LMAX + 1):
                    node = cell >> l
                    outside = np.abs(node[None, :] - node[:, None]) > 1
                    ok = d2 >= r['radius2'][:, l][:, None]
                    assert (ok | ~outside).all(), (name, origin.tolist(), a, l)
                    assert not np.isnan(r['radius2'][:, l]).any()
                    checked += int(outside.sum())
    assert checked > 1_000_000


@pytest.fixture(scope='module')
def all_codes():
    """Morton code of every cell, [512, 512, 64]"""
    out = np.zeros(NB, np.uint32)
    for x0 in range(0, NB[0], 64):
        g = np.stack(np.meshgrid(np.arange(x0, x0 + 64), np.arange(NB[1]), np.arange(NB[2]), indexing='ij'), -1).reshape(-1, 3)
        out[x0:x0 + 64] = mr.probe(cells=g.astype(np.int32), origin=np.zeros(3))['code'].reshape(64, NB[1], NB[2])
    return out


def test_code_is_a_bijection_and_cubes_are_contiguous(all_codes):
    ncodes = NB[0] * NB[1] * NB[2]
    flat = all_codes.reshape(-1).astype(np.int64)
    assert flat.max() == ncodes - 1
    inv = np.full(ncodes, -1, np.int64)
    inv[flat] = np.arange(ncodes)                                    # linear cell index of every code
    assert (inv >= 0).all()                                          # onto, hence one to one
    cz = inv % NB[2]
    cy = (inv // NB[2]) % NB[1]
    cx = inv // (NB[2] * NB[1])
    for l in range(1, mr.LMAX + 1):
        key = ((cx >> l) * (NB[1] >> l) + (cy >> l)) * (NB[2] >> l) + (cz >> l)          # the 2^l-aligned cube of the cell behind each code
        rows = key.reshape(-1, 8 ** l)                                # consecutive runs of 8^l codes
        assert (rows == rows[:, :1]).all(), l                         # one cube per run ...
        assert len(np.unique(rows[:, 0])) == len(rows), l             # ... and one run per cube


def test_level_tables_are_disjoint_and_sized():
    """level l = 1 .. 6 holds (2^24 >> 3l) + 1 entries (the last one is the end of the last node), back to back"""
    off = mr.probe(points=np.zeros((1, 3), F32), origin=np.zeros(3))['lvl_off']
    ncodes = NB[0] * NB[1] * NB[2]
    assert off[0] == 0 and off[1] == 0
    for l in range(1, mr.LMAX + 1):
        assert off[l + 1] - off[l] == (ncodes >> (3 * l)) + 1, l


def test_origin_rule_and_probe_arguments():
    """the two branches of the origin rule (centred when the span fits, anchored at the minimum otherwise), a multiple of 0.4 each time"""
    lo = F32([-37.58, -37.58, -37.58])        # 0.02 above a face: centring by half of 0.1 m crosses it
    for span, centred in ((204.7, True), (204.9, False)):
        o = mr.probe(points=np.zeros((1, 3), F32), bbox=(lo, lo + F32([span, 1, 1])))['origin'][0]
        assert (o == np.floor(float(lo[0]) / 0.4) * 0.4) == (not centred)
        assert abs((o / 0.4) - round(o / 0.4)) < 1e-9
    for span, centred in ((25.5, True), (25.7, False)):
        o = mr.probe(points=np.zeros((1, 3), F32), bbox=(lo, lo + F32([1, 1, span])))['origin'][2]
        assert (o == np.floor(float(lo[0]) / 0.4) * 0.4) == (not centred)
    from vilgod_amd._lib import lib
    assert lib.vg_cluster_geom_probe(None, None, None, None, None, 0, None, None, None, None, None, None) != 0       # neither origin nor box
    bad = np.array([[0, 0, 64]], np.int32)
    o = np.zeros(3)
    assert lib.vg_cluster_geom_probe(mr._p(o), None, None, None, None, 1, None, mr._p(bad), None, None, None, None) != 0  # cell beyond the grid


def test_round_counter_on_known_inputs():
    """the plain Boruvka of mst_ref: a ruler line of 2^m points takes m rounds, a line of growing gaps one"""
    R = mr.ruler_scene(64)
    assert mr.boruvka_rounds(R, ho.core_distances_sq(R, 1)) == 6
    F = mr.few_rounds_scene(100)
    assert mr.boruvka_rounds(F, ho.core_distances_sq(F, 1)) == 1


def test_lattice_scenes_are_aimed():
    """the guard against vacuous scenes, checkable without a GPU as well (the GPU tests assert it again)"""
    seen = set()
    for name in mr.LATTICE_NAMES:
        X, axes = mr.lattice_scene(name)
        got = {a for a, _, _ in mr.parent_violations(X)}
        assert got == set(axes), (name, got)
        seen |= got
    assert seen == {0, 1, 2}
    assert np.abs(mr.lattice_scene('beyond400_x_025')[0][:, 0]).min() > 400


# ================================================================================================ GPU: scenes per pruning rule
MAX_POINTS = 8192
KS = (15, 1)


@pytest.fixture(scope='module')
def models(cuda):
    """one handle per (min_samples, hierarchy), reused by every scene of this module (itself a test of reuse; `test_handle_reuse`
    compares with fresh handles)"""
    from vilgod_amd.hdbscan import HDBSCAN
    cache = {}

    def get(k, hierarchy='host'):
        if (k, hierarchy) not in cache:
            cache[(k, hierarchy)] = HDBSCAN(cluster_selection_epsilon=0.15, min_cluster_size=15, min_samples=k, metric='euclidean',
                                            core_dist_n_jobs=-1, max_points=MAX_POINTS, device=cuda, hierarchy=hierarchy)
        return cache[(k, hierarchy)]
    return get


@pytest.fixture(scope='module')
def oracle():
    """(core2, sorted edges, sorted weights, labels, probabilities) of a point array, computed once per array and shared"""
    cache = {}

    def get(X, k):
        key = (X.tobytes(), X.shape, k)
        if key not in cache:
            core2 = ho.core_distances_sq(X, k)
            edges, w2 = (ho.mst_prim if len(X) <= 1500 else ho.mst_prim_c)(X, core2)
            e, w2s = ho.sort_edges(edges, w2)
            lab, prob = ho.tree_from_mst(e, w2s, len(X))
            for a in (core2, e, w2s, lab, prob):
                a.setflags(write=False)
            cache[key] = (core2, e, w2s, lab, prob)
        return cache[key]
    return get


def check_exact(cuda, models, oracle, X, k, perms=3):
    """-> rounds of each run.  X [n, 3..5] float32; every column is a clustering coordinate."""
    import torch
    X = np.ascontiguousarray(X, F32)
    n, dim = X.shape
    assert 2 <= n <= MAX_POINTS
    rounds = []
    for seed in range(perms):
        Xp = np.ascontiguousarray(X[np.random.default_rng(seed).permutation(n)])
        want_core2, e, w2s, want_l, want_p = oracle(Xp, k)
        model = models(k)
        lo, hi, w2, core2 = [t.cpu().numpy() for t in model.mst(torch.from_numpy(Xp).to(cuda), want_core=True, dim=dim)]
        rounds.append(model.n_rounds_)
        assert np.array_equal(core2, want_core2), (seed, 'core2')
        assert np.array_equal(w2, w2s), (seed, 'weights')
        got = np.stack([lo, hi], 1)[np.lexsort((hi, lo, w2))]
        assert np.array_equal(got, e), (seed, 'edges')
        for hierarchy in ('host', 'device'):
            m = models(k, hierarchy).fit(Xp)
            assert np.array_equal(m.labels_, want_l), (seed, hierarchy, 'labels')
            assert np.array_equal(m.probabilities_, want_p), (seed, hierarchy, 'probabilities')
    return rounds


# ---- a. face-aligned lattices
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', mr.LATTICE_NAMES)
def test_face_aligned_lattice(cuda, models, oracle, name, k):
    X, axes = mr.lattice_scene(name)
    assert {a for a, _, _ in mr.parent_violations(X)} == set(axes)       # the scene is aimed (mst_ref._LATTICES on the one without axes)
    check_exact(cuda, models, oracle, X, k)


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('kind', ['e_const', 'e_vary', '5d'])
@pytest.mark.parametrize('name', mr.LATTICE_NAMES)
def test_face_aligned_lattice_4d_5d(cuda, models, oracle, name, kind, k):
    X, axes = mr.lattice_scene(name)
    assert {a for a, _, _ in mr.parent_violations(X)} == set(axes)
    check_exact(cuda, models, oracle, mr.with_extra_coords(X, kind), k)


# ---- b. the largest component sits a round out from n / 8 points
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', ['below', 'at', 'above', 'two_equal', 'two_equal_at'])
def test_sit_out_threshold(cuda, models, oracle, case, k):
    n = 800
    if case in ('below', 'at', 'above'):
        X = mr.sitout_scene(n, n // 8 + {'below': -1, 'at': 0, 'above': 1}[case])
    else:
        X = mr.sitout_scene(n, 160 if case == 'two_equal' else n // 8, blobs=2)       # equal sizes: the root id decides
    blob = {'below': n // 8 - 1, 'at': n // 8, 'above': n // 8 + 1, 'two_equal': 160, 'two_equal_at': n // 8}[case]
    # the scene is aimed: some round ends with the largest component at exactly the blob's size (until a component reaches n / 8 points
    # nothing sits out, so up to that round the kernels' rounds are the plain ones)
    assert blob in mr.boruvka_largest(X, ho.core_distances_sq(X, k)), case
    check_exact(cuda, models, oracle, X, k)


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', [16, 17, 23, 24])
def test_sit_out_tiny_n(cuda, models, oracle, n, k):
    check_exact(cuda, models, oracle, mr.tiny_scene(n), k)


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
def test_sit_out_blob_among_outlier_pairs(cuda, models, oracle, k):
    check_exact(cuda, models, oracle, mr.outlier_pairs_scene(), k)


# ---- c. purity tables
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', ['slabs_level3', 'slabs_level1', 'enclosed', 'sheet'])
def test_purity_tables(cuda, models, oracle, case, k):
    X = {'slabs_level3': lambda: mr.slabs_scene(3), 'slabs_level1': lambda: mr.slabs_scene(1), 'enclosed': mr.enclosed_scene,
         'sheet': mr.sheet_scene}[case]()
    check_exact(cuda, models, oracle, X, k)


# ---- d. many rounds, kept candidates, queued rounds
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['ruler', 'comb'])
def test_many_rounds(cuda, models, oracle, case):
    """more rounds than the first queued batch of 6: the batch boundary, one round at a time behind it, the counter ring"""
    X = mr.ruler_scene(1024) if case == 'ruler' else mr.comb_scene()
    assert mr.boruvka_rounds(X, ho.core_distances_sq(X, 1)) >= 8
    rounds = check_exact(cuda, models, oracle, X, 1)
    print(f'{case}: rounds on the GPU {rounds}')
    assert min(rounds) > 6


@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
def test_few_rounds(cuda, models, oracle, k):
    """done in <= 3 rounds: the rest of the queued batch are no-ops behind flags[1]"""
    X = mr.few_rounds_scene()
    assert mr.boruvka_rounds(X, ho.core_distances_sq(X, k)) <= 3
    rounds = check_exact(cuda, models, oracle, X, k)
    print(f'few rounds, k={k}: rounds on the GPU {rounds}')
    assert max(rounds) < 6


# ---- e. beyond the grid
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('case', ['ring', 'column', 'six_sides', 'x_under', 'x_over', 'y_under', 'y_over', 'z_under', 'z_over'])
def test_beyond_the_grid(cuda, models, oracle, case, k):
    if case in ('ring', 'column', 'six_sides'):
        X = {'ring': mr.ring_scene, 'column': mr.column_scene, 'six_sides': mr.six_sides_scene}[case]()
    else:
        axis = 'xyz'.index(case[0])
        ext = mr.EXT[axis]
        X = mr.span_scene(axis, ext - 0.1 if case.endswith('under') else ext + 0.1)
        o = mr.probe(points=X[:1], bbox=mr.bbox_of(X))['origin'][axis]
        assert (o == np.floor(float(X[:, axis].min()) / 0.4) * 0.4) == case.endswith('over')      # the branch of the origin rule
    check_exact(cuda, models, oracle, X, k)


# ---- f. launch edges
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', [63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025])
def test_launch_edges(cuda, models, oracle, n, k):
    check_exact(cuda, models, oracle, mr.launch_scene(n), k)


# ---- g. handle reuse
@pytest.mark.gpu
def test_handle_reuse_across_dimensions(cuda):
    """5-D, another 4-D, a 3-D scene and the first again on ONE handle: each equals a fresh handle's result bit for bit (stale cell_e,
    purity or cell-start entries would show)"""
    import torch
    from vilgod_amd.hdbscan import HDBSCAN

    def new():
        return HDBSCAN(cluster_selection_epsilon=0.15, min_cluster_size=15, metric='euclidean', max_points=MAX_POINTS, device=cuda)

    def run(model, X):
        lo, hi, w2, core2 = [t.cpu().numpy() for t in model.mst(torch.from_numpy(X).to(cuda), want_core=True, dim=X.shape[1])]
        order = np.lexsort((hi, lo, w2))
        m = model.fit(X)
        return lo[order], hi[order], w2[order], core2, m.labels_.copy(), m.probabilities_.copy()
    a = mr.with_extra_coords(mr.lattice_scene('x_0125')[0], '5d')
    b = mr.with_extra_coords(mr.sheet_scene() + F32([3.3, -1.7, 0.2]), 'e_vary')
    c = mr.six_sides_scene()
    one = new()
    for i, X in enumerate((a, b, c, a)):
        got, want = run(one, X), run(new(), X)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), i


# ---- h. the range of the 4th coordinate
@pytest.mark.gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('kind', ['tiny', 'huge', 'fine'])
def test_fourth_coordinate_beyond_fp16(cuda, models, oracle, kind, k):
    """the per-node (min, max) of the 4th coordinate is kept as two fp16: values fp16 cannot hold (1e-9, +-70000) or resolve (2^-14 around
    1.0) must only loosen the bound.  Spatially coincident points differ in the 4th coordinate alone."""
    check_exact(cuda, models, oracle, mr.fourth_range_scene(kind), k)
