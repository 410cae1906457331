"""Inputs, a plain round counter and the grid-geometry probe for the Boruvka MST of csrc/cluster_mst.inc (geometry: cluster_geom.inc).  TEST INFRASTRUCTURE ONLY.

Three things live here:
  * `probe`: the host-only C entry vg_cluster_geom_probe -- the origin, cells, Morton codes, box distances and shell radii the kernels
    prune with, evaluated on the CPU by the very functions they call.  Expected values never come from it: the tests compare it with
    the float64 pair distance and with plain integer arithmetic.
  * `parent_*`: the formulas cluster.hip used BEFORE cells were assigned by the computed faces (cell = floor((x - o) * 2.5), box =
    [o + c * s, (o + c * s) + s]), restated in numpy float64 (the file is compiled with -ffp-contract=off, so numpy reproduces them).
    They are kept for ONE purpose: choosing lattice translations at which those formulas put a point outside its own box, so that the
    scenes are aimed at the defect and stay aimed at it.  No expected value depends on them.
  * scene builders, one family per pruning rule, and `boruvka_rounds`, a dense Boruvka without any of the kernels' shortcuts, used only
    to choose sizes that need more rounds than the first queued batch.
"""
import ctypes
import functools

import numpy as np

import neighbors_ref as nr

F32 = np.float32
CELL = nr.CELL
NB = nr.NB
EXT = nr.EXT
LMAX = 6
ANCHORS = nr.OFFSETS                                  # the anchors tests/test_neighbors_edges.py uses


# ------------------------------------------------------------------------------------------------------------ the probe
def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def probe(points=None, queries=None, bbox=None, origin=None, cells=None, want_code=True):
    """vg_cluster_geom_probe.  Exactly one of `bbox` ((lo [3], hi [3]) float32 extremes) / `origin` ([3] float64); `points` [n,3]
    float32 or `cells` [n,3] int32; `queries` [n,3] float32 or None.  -> dict(origin, cell, code, box_d2 [n,7], radius2 [n,7], lvl_off)."""
    from vilgod_amd._lib import lib
    if points is not None:
        points = np.ascontiguousarray(points, F32)
        n = len(points)
        cell = np.zeros((n, 3), np.int32)
    else:
        cell = np.ascontiguousarray(cells, np.int32)
        n = len(cell)
    if queries is not None:
        queries = np.ascontiguousarray(queries, F32)
        assert queries.shape == (n, 3)
    o_in = None if origin is None else np.ascontiguousarray(origin, np.float64)
    lo = hi = None
    if bbox is not None:
        lo, hi = np.ascontiguousarray(bbox[0], F32), np.ascontiguousarray(bbox[1], F32)
    out_o = np.zeros(3)
    code = np.zeros(n, np.uint32) if want_code else None
    box = np.zeros((n, LMAX + 1)) if queries is not None else None
    rad = np.zeros((n, LMAX + 1)) if queries is not None else None
    lvl = np.zeros(LMAX + 2, np.int64)
    rc = lib.vg_cluster_geom_probe(_p(o_in), _p(lo), _p(hi), _p(points), _p(queries), n, _p(out_o), _p(cell), _p(code), _p(box), _p(rad),
                                   _p(lvl))
    assert rc == 0, rc
    return dict(origin=out_o, cell=cell, code=code, box_d2=box, radius2=rad, lvl_off=lvl)


def bbox_of(X):
    X = np.asarray(X, F32)[:, :3]
    return X.min(0), X.max(0)


def d2_f64(q, p):
    """the kernels' pair distance: float64 (dx*dx + dy*dy) + dz*dz of exactly converted float32 coordinates"""
    d = np.asarray(q, F32).astype(np.float64) - np.asarray(p, F32).astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def steps(v, k):
    """float32 value k steps from v (k may be an array)"""
    v = np.asarray(v, F32)
    i = v.view(np.int32).astype(np.int64)
    i = np.where(i < 0, np.int64(-(1 << 31)) - i, i)                 # sign-magnitude -> ordered integers
    i = i + k
    i = np.where(i < 0, np.int64(-(1 << 31)) - i, i)
    return i.astype(np.int32).view(F32)


def face_values(origin, axis, faces=None):
    """float32 values 0, +-1, +-2 steps from the faces o + i * 0.4 of one axis (all faces, or the given face numbers)"""
    i = np.arange(NB[axis] + 1) if faces is None else np.asarray(faces)
    f = (origin[axis] + i.astype(np.float64) * CELL).astype(F32)
    return np.unique(np.concatenate([steps(f, k) for k in (-2, -1, 0, 1, 2)]))


def outside_values(origin, axis):
    """float32 coordinates beyond the grid on both sides of one axis (such points are clamped into the border cells)"""
    lo, hi = origin[axis], origin[axis] + EXT[axis]
    return np.array([lo - 300.0, lo - 5.0, lo - 1e-3, hi + 1e-3, hi + 5.0, hi + 300.0], F32)


# ------------------------------------------------------------------------------------------------------------ parent formulas (scene choice only)
def parent_origin(X):
    return nr.grid_origin(X)


def parent_cell(v, o, n):
    """the earlier cell rule of one axis: floor((v - o) * (1 / 0.4)), clamped"""
    return np.clip(np.floor((np.asarray(v, np.float64) - o) * (1.0 / CELL)).astype(np.int64), 0, n - 1)


def parent_outside_axis(v, o, n, level):
    """-> (below, above): which float32 coordinates v of one axis lie outside the earlier box of their own level-`level` node:
    box = [lo, lo + s] with lo = o + c * s, s = 0.4 * 2^level (border nodes are open outwards)."""
    v = np.asarray(v, F32).astype(np.float64)
    c = parent_cell(v, o, n) >> level
    s = CELL * float(1 << level)
    lo = o + c.astype(np.float64) * s
    hi = lo + s
    return (v < lo) & (c > 0), (v > hi) & (c < (n >> level) - 1)


def parent_box_d2(origin, q, p, level):
    """the earlier cl_box_d2 from queries q to the level-`level` nodes that the earlier cell rule gives points p ([m,3] float32 each)"""
    q, p = np.asarray(q, F32).astype(np.float64), np.asarray(p, F32).astype(np.float64)
    s = CELL * float(1 << level)
    d2 = np.zeros(len(p))
    for a in range(3):
        c = parent_cell(p[:, a], origin[a], NB[a]) >> level
        lo = origin[a] + c.astype(np.float64) * s
        hi = lo + s
        d = np.where((q[:, a] < lo) & (c > 0), lo - q[:, a], np.where((q[:, a] > hi) & (c < (NB[a] >> level) - 1), q[:, a] - hi, 0.0))
        d2 = d2 + d * d
    return d2


def parent_violations(X, levels=(0, 1)):
    """Points of X ([n,>=3] float32) that the earlier formulas leave outside their own box although occupied cells lie beyond that
    face (a query there gets a box distance LARGER than its distance to the point).  -> list of (axis, level, point row)."""
    X = np.asarray(X, F32)
    o = parent_origin(X)
    out = []
    for a in range(3):
        c0 = parent_cell(X[:, a].astype(np.float64), o[a], NB[a])
        for l in levels:
            below, above = parent_outside_axis(X[:, a], o[a], NB[a], l)
            c = c0 >> l
            for i in np.flatnonzero(below):
                if (c < c[i]).any():
                    out.append((a, l, int(i)))
            for i in np.flatnonzero(above):
                if (c > c[i]).any():
                    out.append((a, l, int(i)))
    return out


def _axis_run(start, spacing, count):
    return (np.float64(start) + np.arange(count) * np.float64(spacing)).astype(F32)


@functools.lru_cache(maxsize=None)
def find_start(axis, spacing, count, lo=-200.0, hi=200.0, want=True):
    """First start in arange(lo, hi, 0.5) at which a run of `count` coordinates at `spacing` along `axis` has (want=True) / has not
    (want=False) a point outside its earlier level-0 or level-1 box with occupied cells beyond the face."""
    for s in np.arange(lo, hi, 0.5):
        v = _axis_run(s, spacing, count)
        X = np.zeros((count, 3), F32)
        X[:, axis] = v
        o = parent_origin(X)[axis]
        hit = False
        for l in (0, 1):
            below, above = parent_outside_axis(v, o, NB[axis], l)
            c = parent_cell(v.astype(np.float64), o, NB[axis]) >> l
            hit = hit or any((c < c[i]).any() for i in np.flatnonzero(below)) or any((c > c[i]).any() for i in np.flatnonzero(above))
        if hit == want:
            return float(s)
    raise AssertionError('no such start')


def lattice(spacing, counts, starts):
    ax = [_axis_run(starts[a], spacing, counts[a]) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    return np.ascontiguousarray(g, F32)


# name -> (spacing, counts, axes that must violate, start ranges of those axes, doubled)
_LATTICES = {
    'x_0125': (0.125, (16, 8, 8), (0,), {}, False),
    'x_0125_4k': (0.125, (32, 16, 8), (0,), {}, False),           # 4 096 points: level-2 and level-3 nodes above the leaf size
    'y_025': (0.25, (12, 12, 8), (1,), {}, False),
    'z_05': (0.5, (12, 12, 6), (2,), {}, False),
    'z_0125': (0.125, (8, 8, 12), (2,), {}, False),
    'far_x_025': (0.25, (12, 10, 8), (0,), {0: (120.0, 128.0)}, False),       # the farthest a centred lattice can be: see `beyond400_x_025`
    # |x| > 400 m.  The earlier formulas put NO lattice point outside its box there (the spacing of float64 at 256 m and beyond,
    # 5.7e-14, swallows the error of o + i * 0.4; the farthest violation of any origin sits at |x| = 254 m, of a lattice centred in
    # its grid below 128 m), so this scene runs
    # without the guard: face-aligned points (even integers are faces) far from the origin, exact like the others.
    'beyond400_x_025': (0.25, (12, 10, 8), (), {0: (480.0, 900.0)}, False),
    'xyz_025': (0.25, (10, 10, 6), (0, 1, 2), {}, False),
    'doubled_y_0125': (0.125, (6, 16, 5), (1,), {}, True),
}
LATTICE_NAMES = tuple(_LATTICES)


@functools.lru_cache(maxsize=None)
def lattice_scene(name):
    """-> (X [n,3] float32, axes that the earlier formulas violate).  The other axes start where they do NOT violate, so that each
    scene names its axis."""
    spacing, counts, axes, ranges, doubled = _LATTICES[name]
    starts = []
    for a in range(3):
        lo, hi = ranges.get(a, (-200.0, 200.0))
        starts.append(find_start(a, spacing, counts[a], lo, hi, want=a in axes))
    X = lattice(spacing, counts, starts)
    if doubled:
        X = np.concatenate([X, X])
    X.setflags(write=False)
    return X, axes


def with_extra_coords(X, kind):
    """the same points in 4-D / 5-D: 'e_const' (4th = 0.5), 'e_vary' (five levels 0.05 apart), '5d' (+ 0.1 * frame)"""
    n = len(X)
    i = np.arange(n)
    if kind == 'e_const':
        return np.concatenate([X, np.full((n, 1), 0.5, F32)], 1)
    e = ((i * 7) % 5).astype(F32)[:, None] * F32(0.05)
    if kind == 'e_vary':
        return np.concatenate([X, e], 1)
    assert kind == '5d'
    return np.concatenate([X, e, ((i // 3) % 2).astype(F32)[:, None] * F32(0.1)], 1)


# ------------------------------------------------------------------------------------------------------------ a plain Boruvka round counter
def boruvka_rounds(X, core2):
    return len(boruvka_largest(X, core2))


def boruvka_largest(X, core2):
    """Size of the largest component after each round of textbook Boruvka (EVERY component picks its minimum leaving edge under (w2, d2, lo, hi) each round: no sit-out, no
    kept candidates, no bounds) on the dense mutual-reachability graph of X.  n up to a few thousand."""
    X = np.ascontiguousarray(X, np.float64)
    n = len(X)
    d = X[:, None, :] - X[None, :, :]
    d2 = d[..., 0] * d[..., 0]
    for c in range(1, X.shape[1]):
        d2 = d2 + d[..., c] * d[..., c]
    w = np.maximum(np.maximum(d2, core2[:, None]), core2[None, :])
    iu, ju = np.triu_indices(n, 1)
    order = np.lexsort((ju, iu, d2[iu, ju], w[iu, ju]))
    rank = np.full((n, n), np.iinfo(np.int64).max, np.int64)
    rank[iu[order], ju[order]] = np.arange(len(order))
    rank = np.minimum(rank, rank.T)
    comp = np.arange(n)
    largest = []
    while len(np.unique(comp)) > 1:
        r = np.where(comp[:, None] == comp[None, :], np.iinfo(np.int64).max, rank)
        best_j = r.argmin(1)
        best_r = r[np.arange(n), best_j]
        cb = np.full(n, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(cb, comp, best_r)
        pick = np.flatnonzero(best_r == cb[comp])                     # one point per component (ranks are unique per edge; both ends may pick it)
        parent = np.arange(n)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for i in pick:
            a, b = find(comp[i]), find(comp[best_j[i]])
            if a != b:
                parent[max(a, b)] = min(a, b)
        comp = np.array([find(c) for c in comp])
        largest.append(int(np.bincount(comp).max()))
    return largest


# ------------------------------------------------------------------------------------------------------------ scenes per rule
def _groups(rng, total):
    """`total` points in groups of 1 .. 20 on the nodes of a 5 m grid that starts 25 m from the blobs: every point's nearest foreign
    point is in another group, never in a blob, so the blobs unite on their own before anything joins them"""
    out, node = [], 0
    while total > 0:
        m = int(min(rng.integers(1, 21), total))
        c = np.array([25.0 + 5.0 * (node % 12), -30.0 + 5.0 * (node // 12), 0.0])
        out.append(c + rng.normal(size=(m, 3)) * [0.15, 0.15, 0.05])
        total -= m
        node += 1
    return out


def sitout_scene(n, blob, seed=2, blobs=1):
    """one (or two equal) dense blob(s) of exactly `blob` points + groups of 1 .. 20 points: n points in all.  The tests assert with
    `boruvka_largest` that some round ends with the largest component at exactly `blob` points."""
    rng = np.random.default_rng(seed)
    parts = [rng.normal(size=(blob, 3)) * 0.05 + [k * 9.0, 0, 0] for k in range(blobs)]
    parts += _groups(rng, n - blob * blobs)
    X = np.concatenate(parts).astype(F32)
    assert len(X) == n
    return X


def tiny_scene(n, seed=0):
    """n = 16, 17, 23, 24: where max(2, n / 8) rounds -- a blob of n / 2 points and single points around it"""
    rng = np.random.default_rng(100 + seed)
    m = n // 2
    return np.concatenate([rng.normal(size=(m, 3)) * 0.1, rng.uniform(-6, 6, size=(n - m, 3)) * [1, 1, 0.1]]).astype(F32)


def outlier_pairs_scene(seed=0):
    """a blob surrounded by outliers whose nearest neighbour is ANOTHER OUTLIER (pairs 0.3 m apart, 8 .. 15 m from the blob)"""
    rng = np.random.default_rng(seed)
    blob = rng.normal(size=(300, 3)) * 0.4
    ang = rng.uniform(0, 2 * np.pi, 40)
    r = rng.uniform(8, 15, 40)
    a = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-0.5, 0.5, 40)], 1)
    b = a + rng.normal(size=(40, 3)) * 0.15
    return np.concatenate([blob, a, b]).astype(F32)


def _face_of(X, axis, level, index):
    """coordinate (float64) of face `index` of level `level` on `axis` in the grid the kernels build for X"""
    o = probe(points=X[:1, :3], bbox=bbox_of(X))['origin']
    return o[axis] + index * (CELL * (1 << level))


def slabs_scene(level, seed=0):
    """two dense slabs of different density that meet exactly at a level-`level` node face of x: the x extremes are pinned so that the
    data's centre is 0.2 and the origin -102.4, which puts face 256 (a face of every level up to 6) at x = 0.0.  Slab a ends at the
    last float32 below 0, slab b starts at 0.0; asserted through the probe."""
    rng = np.random.default_rng(seed)
    w = CELL * (1 << level)
    na, nb_ = 700, 350
    X = np.concatenate([rng.uniform([-0.9 * w, 0, 0], [0, 2.0, 0.8], size=(na, 3)),
                        rng.uniform([0, 0, 0], [0.9 * w + 0.4, 2.0, 0.8], size=(nb_, 3))]).astype(F32)
    X[0, 0], X[1, 0] = -0.9 * w, steps(F32(0), -1)
    X[na, 0], X[na + 1, 0] = 0.9 * w + 0.4, 0.0
    X[:na, 0] = np.minimum(X[:na, 0], steps(F32(0), -1))
    r = probe(points=X, bbox=bbox_of(X))
    node = r['cell'][:, 0] >> level
    assert node[:na].max() + 1 == node[na:].min() == 256 >> level and X[na:, 0].min() == 0, (r['origin'], np.unique(node))
    return X


def enclosed_scene(seed=0):
    """a compact dense core (one component early, owning whole level-0..2 nodes) inside a sparse shell that surrounds it on all sides"""
    rng = np.random.default_rng(seed)
    core = rng.uniform(-0.6, 0.6, size=(900, 3))
    v = rng.normal(size=(500, 3))
    shell = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.6, 2.2, size=(500, 1))
    return np.concatenate([core, shell]).astype(F32)


def sheet_scene(seed=0):
    """a dense block cut by a thin, sparser foreign sheet (0.02 m thick, 0.3 m of empty space on either side)"""
    rng = np.random.default_rng(seed)
    left = rng.uniform([-1.6, -1.6, -0.8], [-0.3, 1.6, 0.8], size=(700, 3))
    right = rng.uniform([0.3, -1.6, -0.8], [1.6, 1.6, 0.8], size=(700, 3))
    sheet = rng.uniform([-0.01, -1.6, -0.8], [0.01, 1.6, 0.8], size=(150, 3))
    return np.concatenate([left, right, sheet]).astype(F32)


def ruler_scene(n, base=0.05):
    """a line whose gap i is base * (1 + trailing zero bits of i): with min_samples = 1 textbook Boruvka joins pairs, then pairs of
    pairs, ...: log2(n) rounds"""
    i = np.arange(1, n)
    tz = np.zeros(n - 1, np.int64)
    for b in range(1, 20):
        tz += (i % (1 << b)) == 0
    x = np.concatenate([[0.0], np.cumsum(base * (1 + tz))])
    return np.stack([x, np.zeros(n), np.zeros(n)], 1).astype(F32)


def comb_scene(teeth=64, per_tooth=8, base=0.05):
    """a 2-D comb: a ruler line along x as the spine, a ruler tooth along y on each of its points"""
    spine = ruler_scene(teeth, base * 4)
    tooth = ruler_scene(per_tooth + 1, base)[1:, 0]
    pts = [spine]
    for s in spine:
        t = np.tile(s, (per_tooth, 1))
        t[:, 1] = tooth
        pts.append(t)
    return np.concatenate(pts).astype(F32)


def few_rounds_scene(n=300):
    """a line whose gaps grow strictly from left to right: at min_samples = 1 every point's nearest neighbour is its left one"""
    x = np.cumsum(0.02 * (1.0 + 0.01 * np.arange(n)))
    return np.stack([x, np.zeros(n), np.zeros(n)], 1).astype(F32)


def ring_scene(seed=0):
    """hundreds of points clamped on the four x/y sides: a ring of radius 300 m (the grid spans 204.8 m), a little noise"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, 600)
    return np.stack([300 * np.cos(a), 300 * np.sin(a), rng.normal(size=600) * 0.3], 1).astype(F32)


def column_scene(seed=0):
    """a 60 m tall column (the grid spans 25.6 m in z and is then anchored at the minimum: everything above is clamped)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(size=500) * 0.3, rng.normal(size=500) * 0.3, rng.uniform(-30, 30, 500)], 1).astype(F32)


def six_sides_scene(seed=0):
    """a populated grid + groups far beyond it on all six sides + a dense cluster wholly inside ONE border cell (beyond the grid)"""
    rng = np.random.default_rng(seed)
    inside = rng.uniform([-100, -100, -12], [100, 100, 12], size=(500, 3))
    far = []
    for a in range(3):
        for s in (-1, 1):
            c = np.zeros(3)
            c[a] = s * (260.0 if a < 2 else 45.0)
            far.append(c + rng.normal(size=(60, 3)) * [2.0, 2.0, 0.5])
    dense = np.array([400.0, 400.0, 50.0]) + rng.normal(size=(200, 3)) * 0.05
    return np.concatenate([inside] + far + [dense]).astype(F32)


def span_scene(axis, span, seed=0):
    """groups spread over exactly `span` metres of one axis (two points pin the extremes): just under / over the grid's extent takes
    the two branches of the origin rule"""
    rng = np.random.default_rng(seed)
    n = 400
    X = rng.uniform([-20, -20, -2], [20, 20, 2], size=(n, 3))
    X[:, axis] = rng.uniform(0, span, n)
    X[0, axis], X[1, axis] = 0.0, span
    X = X.astype(F32)
    X[:, axis] += F32(-37.58)               # 0.02 m above a face: centring by 0.05 m crosses it, the two branches differ
    return X


def launch_scene(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    k = max(2, n // 40)
    cents = rng.uniform(-15, 15, size=(k, 3)) * [1, 1, 0.1]
    return (cents[rng.integers(0, k, n)] + rng.normal(size=(n, 3)) * 0.3).astype(F32)


def fourth_range_scene(kind, seed=0):
    """4-D points whose 4th coordinate fp16 cannot hold (1e-9 underflows, +-70000 overflows) or resolve (neighbours 2^-14 apart around
    1.0).  Groups of spatially COINCIDENT points are separated by the 4th coordinate alone."""
    rng = np.random.default_rng(seed)
    sites = rng.uniform([-3, -3, -0.5], [3, 3, 0.5], size=(60, 3)).astype(F32)
    if kind == 'tiny':
        vals = np.array([0.0, 1e-9, 2e-9, 3e-9, -1e-9, 5e-9], F32)
    elif kind == 'huge':
        vals = np.array([70000.0, -70000.0, 69999.0, 0.0, 65504.0, -65520.0], F32)
    else:
        assert kind == 'fine'
        vals = (1.0 + np.arange(-3, 3) * 2.0 ** -14).astype(F32)
    X = np.concatenate([np.repeat(sites, len(vals), 0), np.tile(vals, len(sites))[:, None]], 1).astype(F32)
    return X
