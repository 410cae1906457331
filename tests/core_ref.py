"""Reference, restatement, synthesised faults and aimed scenes for the exact k-NN core distances of csrc/cluster_core.inc (k_cl_blocks,
k_cl_core_blk, k_cl_core_far).  TEST INFRASTRUCTURE ONLY: nothing here calls the GPU.

  * `core2_dense`: the expected value, always.  All pairs in float64 on the exactly widened float32 rows, the row itself excluded by its
    index, no KD-tree and no candidate cut.
  * `Stage` / `Stage.run`: the stage's DECISIONS restated in Python from the cells and codes of the host-only geometry probe
    (mst_ref.probe): the work list (96 / 4096 / 64), the passes over the 128-slot tile, the node skip, done against the shell radius, the
    start and end level of phase B (7 = the scan of all points).  It exists to show that a scene sits where its name says and to describe
    a failing row; with a `fault` it returns the wrong answer that slip would give, so that the scenes can be shown to notice it.
  * scene families, placed with the probe: `cases(family)` lists (case, dim, k), `scene` builds the float32 rows.
"""
import collections
import functools
import itertools

import numpy as np

import mst_ref as mr

F32 = np.float32
CELL = mr.CELL
NB = mr.NB
LMAX = mr.LMAX
SCAN_ALL = LMAX + 1                   # "level 7": phase B streamed every point
CLB_SPLIT = 96                        # a level-1 node with more points is handled cell by cell
CLB_SHELL_CAP = 4096                  # ... and so is one whose level-3 ancestor holds more
CHUNK = 64                            # queries per work item
CLB_TILE = 128                        # candidates staged per pass
CL_K = 16                             # k < 16: register list / 16-lane row; k >= 16: LDS heap / the whole wave
CLB_ORDER = ([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1),
              (-1, -1, 0), (1, -1, 0), (-1, 1, 0), (1, 1, 0), (-1, 0, -1), (1, 0, -1), (-1, 0, 1), (1, 0, 1), (0, -1, -1), (0, 1, -1), (0, -1, 1),
              (0, 1, 1)] + [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)])
assert len(CLB_ORDER) == 27 and len(set(CLB_ORDER)) == 27
K6 = (1, 15, 16, 32, 33, 64)
K10 = (1, 8, 15, 16, 17, 32, 33, 48, 49, 64)
FAULTS = {                            # fault -> the family whose cases have to notice it
    'drop_straddle': 'tile',          # the remainder of a node that straddles a tile is dropped
    'chunk_reads_first': 'node_m',    # the second chunk of a node reads the first chunk's queries
    'skip_any': 'tile',               # a node is skipped once its box is >= ONE live lane's k-th distance (the rule: >= EVERY lane's)
    'done_coarser': 'shell_edge',     # done is decided against the radius one level coarser
    'no_reset': 'far_L',              # the list is not reset at ++L
    'no_scan_all': 'far_L',           # the scan of all points is left out
    'lane_low': 'far_L',              # the answer is read one lane low
    'lane_high': 'far_L',             # ... one lane high
    'heap_drops_zeros': 'self',       # the heap form drops every candidate at distance 0 instead of only the first
    'reg_no_self': 'self',            # the register form does not count the query
}


# ------------------------------------------------------------------------------------------------------------ the reference
def _d2(A, B):
    """[a, D] x [b, D] float64 -> [a, b]: ((dx*dx + dy*dy) + dz*dz [+ de*de [+ dt*dt]]), summed left to right"""
    d = A[:, None, :] - B[None, :, :]
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    for c in range(2, A.shape[1]):
        s = s + d[..., c] * d[..., c]
    return s


def core2_dense(X, k, dim, block=256):
    """squared distance to the k-th nearest OTHER row of X[:, :dim] (float32, widened exactly); +inf for n <= k"""
    P = np.ascontiguousarray(np.asarray(X, F32)[:, :dim]).astype(np.float64)
    n = len(P)
    if n <= k:
        return np.full(n, np.inf)
    out = np.empty(n)
    for s in range(0, n, block):
        d2 = _d2(P[s:s + block], P)
        b = len(d2)
        d2[np.arange(b), np.arange(s, s + b)] = np.inf               # the row itself, by index
        out[s:s + b] = np.partition(d2, k - 1, axis=1)[:, k - 1]
    return out


# ------------------------------------------------------------------------------------------------------------ the restatement
Account = collections.namedtuple('Account', 'core2 entries entry_of level kth_a done start end pop straddle n_items n_far order')


class Stage:
    """the grid of one input as the kernels see it: rows in sorted (Morton, then input) order, the nodes of every level as ranges"""

    def __init__(self, X, dim):
        self.dim = dim
        X = np.ascontiguousarray(np.asarray(X, F32)[:, :dim])
        xyz = np.ascontiguousarray(X[:, :3])
        r = mr.probe(points=xyz, queries=xyz, bbox=mr.bbox_of(xyz))
        self.origin = r['origin']
        self.order = np.argsort(r['code'], kind='stable')             # the radix sort is stable
        self.n = len(X)
        self.code = r['code'][self.order]
        self.cell = r['cell'][self.order]
        self.radius2 = r['radius2'][self.order]
        self.xyz = xyz[self.order]
        self.P = X[self.order].astype(np.float64)
        self.nodes = []
        for l in range(LMAX + 1):
            key = self.code >> np.uint32(3 * l)
            first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
            end = np.r_[first[1:], self.n]
            self.nodes.append({tuple(int(v) for v in self.cell[f] >> l): (int(f), int(e)) for f, e in zip(first, end)})
        self._box, self._nbh = {}, {}                                 # (neither depends on k)

    def node_range(self, level, c):
        return self.nodes[level].get(tuple(int(v) for v in c), (0, 0))

    def work_list(self):
        """the rule of k_cl_blocks -> [(level, first sorted index, chunks)]"""
        cells = sorted(self.nodes[0].values())
        out = []
        for c1, (s, e) in sorted(self.nodes[1].items(), key=lambda kv: kv[1]):
            s3, e3 = self.node_range(3, np.array(c1) >> 2)
            if e - s <= CLB_SPLIT and e3 - s3 <= CLB_SHELL_CAP:
                out.append((1, s, (e - s + CHUNK - 1) // CHUNK))
            else:
                out += [(0, s0, (e0 - s0 + CHUNK - 1) // CHUNK) for s0, e0 in cells if s <= s0 < e]
        return out

    def box_d2(self, level, c, rows):
        """cl_box_d2 from the sorted rows to node c of `level` (the probe evaluates the kernels' own function)"""
        cells = np.tile(np.asarray(c, np.int32) << level, (len(rows), 1))
        return mr.probe(cells=cells, queries=self.xyz[rows], origin=self.origin, want_code=False)['box_d2'][:, level]

    def neighbourhood(self, level, c):
        """the 27 ranges around node c in CLB_ORDER; a node beyond the grid is empty"""
        key = (level,) + tuple(int(v) for v in c)
        if key in self._nbh:
            return self._nbh[key]
        out = self._nbh[key] = []
        for o in CLB_ORDER:
            nc = np.asarray(c) + o
            ok = all(0 <= nc[a] < (NB[a] >> level) for a in range(3))
            out.append((tuple(int(v) for v in nc), self.node_range(level, nc) if ok else (0, 0)))
        return out

    # ---- phase A: one work item
    def _phase_a(self, level, i0, k, fault):
        s, e = self.node_range(level, self.cell[i0] >> level)           # the node of code_s[i0]
        rows = np.arange(i0, min(e, i0 + CHUNK))
        src = rows
        if fault == 'chunk_reads_first' and i0 > s:
            src = s + np.arange(len(rows))
        b = self.cell[i0] >> level
        nbh = self.neighbourhood(level, b)
        heap = k >= CL_K
        cap = k if heap else CL_K
        lst = np.full((len(rows), cap), np.inf)
        seen = np.zeros(len(rows), bool)
        kth = lambda: lst[:, k - 1] if heap else lst[:, k]
        boxes = self._box.setdefault((level, i0, fault == 'chunk_reads_first'), {})      # (they do not depend on k)
        t_next, cur, pop, straddle = 0, nbh[0][1][0], 0, False
        while t_next < 27:
            segs, tot = [], 0
            while t_next < 27 and tot < CLB_TILE:
                j1 = nbh[t_next][1][1]
                need = cur < j1
                if need:
                    if t_next not in boxes:
                        boxes[t_next] = self.box_d2(level, nbh[t_next][0], src)
                    need = bool(np.all(boxes[t_next] < kth())) if fault == 'skip_any' else bool(np.any(boxes[t_next] < kth()))
                if need:
                    take = min(j1 - cur, CLB_TILE - tot)
                    segs.append(np.arange(cur, cur + take))
                    tot += take
                    cur += take
                    if cur < j1:
                        straddle = True
                        if fault != 'drop_straddle':
                            break
                t_next += 1
                if t_next < 27:
                    cur = nbh[t_next][1][0]
            if tot == 0:
                break
            cand = np.concatenate(segs)
            D = _d2(self.P[src], self.P[cand])
            if heap:
                zero = D == 0.0
                if fault == 'heap_drops_zeros':
                    D[zero] = np.inf
                else:                                                # the first candidate at exactly 0 stands for the query
                    hit = zero.any(1) & ~seen
                    D[np.flatnonzero(hit), zero.argmax(1)[hit]] = np.inf
                    seen |= hit
            elif fault == 'reg_no_self':
                D[cand[None, :] == src[:, None]] = np.inf
            lst = np.sort(np.concatenate([lst, D], 1), 1)[:, :cap]
            pop += tot
        r2 = self.radius2[src, min(level + 1, LMAX) if fault == 'done_coarser' else level]
        return rows, kth().copy(), kth() <= r2, pop, straddle

    # ---- phase B: one query
    def _phase_b(self, i, bound, k, fault):
        L = 2
        while L < LMAX and not bound <= self.radius2[i, L]:
            L += 1
        if np.isinf(bound):
            L = 3
        start = L
        wide = k >= CL_K
        kl = (k - 1 if wide else k) + {'lane_low': -1, 'lane_high': 1}.get(fault, 0)
        width = 64 if wide else 16
        carried = np.empty(0)
        while True:
            if L > LMAX:
                if fault == 'no_scan_all':
                    return start, L, np.inf
                cand = np.arange(self.n)
            else:
                cand = np.concatenate([np.arange(s, e) for _, (s, e) in self.neighbourhood(L, self.cell[i] >> L)])
            if wide:
                cand = cand[cand != i]                               # the wave-wide form leaves the query out by its index
            vals = np.sort(np.concatenate([carried, _d2(self.P[i:i + 1], self.P[cand])[0]]))[:width]
            T = vals[kl] if 0 <= kl < len(vals) else np.inf
            if L > LMAX or T <= self.radius2[i, L]:
                return start, L, T
            if fault == 'no_reset':
                carried = vals
            L += 1

    def run(self, k, fault=None):
        """-> Account; every per-row array is in INPUT order.  fault=None restates the stage; a fault name returns that slip's answer."""
        n = self.n
        core2 = np.full(n, np.nan)
        kth_a = np.full(n, np.nan)
        done = np.zeros(n, bool)
        level = np.full(n, -1)
        entry_of = np.full(n, -1)
        start = np.zeros(n, int)
        end = np.zeros(n, int)
        entries, pop, straddle = [], [], []
        for lv, first, chunks in self.work_list():
            for c in range(chunks):
                rows, kth, dn, p, st = self._phase_a(lv, first + c * CHUNK, k, fault)
                entry_of[rows], level[rows], kth_a[rows], done[rows] = len(entries), lv, kth, dn
                entries.append((lv, first + c * CHUNK))
                pop.append(p)
                straddle.append(st)
        assert (entry_of >= 0).all()                                 # the work list covers every row exactly once
        core2[:] = kth_a
        for i in np.flatnonzero(~done):
            start[i], end[i], core2[i] = self._phase_b(i, kth_a[i], k, fault)
        inv = np.empty(n, int)
        inv[self.order] = np.arange(n)                               # input row -> sorted index
        g = lambda a: a[inv]
        return Account(g(core2), entries, g(entry_of), g(level), g(kth_a), g(done), g(start), g(end), pop, straddle, len(entries),
                       int((~done).sum()), self.order)


def describe(acc, row):
    """the restatement's account of one input row, for a failure message"""
    e = acc.entry_of[row]
    how = 'done in phase A' if acc.done[row] else f'far: start level {acc.start[row]}, end level {acc.end[row]}'
    return (f'row {row}: item {e} (level {acc.entries[e][0]}, first sorted index {acc.entries[e][1]}, {acc.pop[e]} candidates staged, '
            f'straddle {acc.straddle[e]}), phase A k-th {acc.kth_a[row]!r}, {how}')


# ------------------------------------------------------------------------------------------------------------ placing points
def _frame(half=(40.0, 40.0, 4.0)):
    """two rows that pin the bounding box (everything else lies inside) and the origin the kernels compute from it"""
    hi = np.asarray(half, F32)
    o = mr.probe(points=np.zeros((1, 3), F32), bbox=(-hi, hi))['origin']
    return np.stack([-hi, hi]), o


def _node_lo(o, level, b):
    return o + np.asarray(b, np.float64) * (CELL * (1 << level))


def _home(o, level=1, shift=(0, 0, 0)):
    """a level-`level` node next to the world origin whose index is a multiple of 4 (+ shift): it starts a level-(level+2) node"""
    b = np.floor((0.0 - o) / (CELL * (1 << level))).astype(int)
    return (b >> 2 << 2) + np.asarray(shift)


def _fill(rng, lo, a, b, m):
    """m points uniform in lo + [a, b) per axis (a, b: scalars or [3])"""
    return lo + rng.uniform(np.broadcast_to(a, 3), np.broadcast_to(b, 3), size=(m, 3))


def _background(rng, m, half=(40.0, 40.0, 4.0), keep_out=15.0):
    out = np.zeros((0, 3))
    while len(out) < m:
        p = rng.uniform(-np.asarray(half) * 0.98, np.asarray(half) * 0.98, size=(2 * m, 3))
        out = np.concatenate([out, p[(np.abs(p[:, :2]) > keep_out).any(1)]])
    return out[:m]


def _nd(X3, dim):
    X = np.ascontiguousarray(X3, F32)
    return X if dim == 3 else mr.with_extra_coords(X, 'e_vary' if dim == 4 else '5d')


def _ring(q, R, k, a0=0.1, a1=None):
    a = a0 + (np.arange(k) + 0.5) * ((2 * np.pi if a1 is None else a1 - a0) / k)
    return np.asarray(q, np.float64) + np.stack([R * np.cos(a), R * np.sin(a), np.zeros(k)], 1)


def _radius(X, row):
    """sqrt of the probe's shell radius of one row at levels 0..6 in the grid of X"""
    xyz = np.ascontiguousarray(np.asarray(X, F32)[:, :3])
    r = mr.probe(points=xyz[row:row + 1], queries=xyz[row:row + 1], bbox=mr.bbox_of(xyz))
    return np.sqrt(r['radius2'][0])


# ------------------------------------------------------------------------------------------------------------ the families
NODE_M = (63, 64, 65, 96, 97)
CELL_M = (64, 65, 128, 129)
TILE_P = (127, 128, 129, 256, 257)
FAR_INF = (3, 4, 5, 6, 7)
FAR_FIN3 = (2, 3)                                     # finite bound in 3-D: see `_far`
FAR_FIN4 = (4, 5, 6, 7)                               # ... needs the 4th coordinate


def cases(family):
    """-> [(case, dim, k)]"""
    d345 = (3, 4, 5)
    if family == 'node_m':
        return [(m, d, k) for m in NODE_M for d in d345 for k in K6]
    if family == 'cell_m':
        return [(m, 3, k) for m in CELL_M for k in K6]
    if family == 'shell_cap':
        return [(m, 3, k) for m in (4096, 4097) for k in K6]
    if family == 'tile':
        return [(p, d, 64) for p in TILE_P for d in d345] + [('straddle', d, k) for d in d345 for k in (64, 1)] + [(256, 3, 1)]
    if family == 'shell_edge':
        return ([(v, d, k) for v in ('in', 'out_lo', 'out_hi') for d in d345 for k in K6] + [('xyz_in', d, k) for d in (4, 5) for k in K6])
    if family == 'far_L':
        out = [(('inf', L), 3, k) for L in FAR_INF for k in K10] + [(('fin', L), 3, k) for L in FAR_FIN3 for k in K10]
        out += [(('fin', L), 4, k) for L in FAR_FIN4 for k in K10]
        out += [(('reset', 4), 3, k) for k in K10 if k > 1]          # "at least one and fewer than k" points is empty at k = 1
        return out + [((c, 0), 3, k) for c in ('corner', 'clamped') for k in K10]
    assert family == 'self'
    out = [(('full', e), d, k) for e in (-1, 0, 1) for d in d345 for k in K6]
    return out + [(('xyz', e), d, k) for e in (-1, 0, 1) for d in (4, 5) for k in K6]


FAMILIES = ('node_m', 'cell_m', 'shell_cap', 'tile', 'shell_edge', 'far_L', 'self')
COUNTED = ('node_m', 'cell_m', 'shell_cap', 'far_L')  # families whose item / far counts are read from the library's own line


def _node_m(m):
    rng = np.random.default_rng(m)
    corners, o = _frame()
    lo = _node_lo(o, 1, _home(o) + 1)
    return np.concatenate([corners, _fill(rng, lo, 0.03, 0.77, m), _background(rng, 300)]).astype(F32)


def _cell_m(m):
    rng = np.random.default_rng(1000 + m)
    corners, o = _frame()
    lo = _node_lo(o, 1, _home(o) + 1)
    sib = [lo + CELL * np.array(c) + rng.uniform(0.02, 0.38, 3) for c in itertools.islice(itertools.cycle(
        [c for c in itertools.product((0, 1), repeat=3) if any(c)]), 40)]
    return np.concatenate([corners, _fill(rng, lo, 0.02, 0.38, m), np.array(sib), _background(rng, 20)]).astype(F32)


def _shell_cap(total):
    rng = np.random.default_rng(total)
    corners, o = _frame()
    b1 = _home(o)                                                     # first level-1 node of a level-3 node
    parts = [corners]
    others = [c for c in itertools.product(range(4), repeat=3) if c != (1, 1, 1)]
    for j, c in enumerate(others):
        m = (64 if j < 47 else 63) + (1 if total == 4097 and j == 62 else 0)
        parts.append(_fill(rng, _node_lo(o, 1, b1 + c), 0.02, 0.78, m))
    parts.append(_fill(rng, _node_lo(o, 1, b1 + 1), 0.02, 0.78, 80))  # the chosen node: rows -180 .. -101
    parts.append(_background(rng, 100))
    return np.concatenate(parts).astype(F32)


def _tile(p):
    """the item is the level-1 node A (70 points, rows 2..71); its CLB_ORDER neighbours 1 (-x), 2 (+x), 3 (-y) hold the rest.
    70 + 30 + 28 = 128: a third node of 29 points straddles slot 128 by one point."""
    rng = np.random.default_rng(77 if p == 'straddle' else p)
    corners, o = _frame()
    b1 = _home(o) + 1
    bar = lambda c, m, x=(0.02, 0.78), y=(0.05, 0.35): _fill(rng, _node_lo(o, 1, b1 + c), [x[0], y[0], 0.05], [x[1], y[1], 0.35], m)
    total = 129 if p == 'straddle' else p
    n2 = 29 if total == 129 else min(total - 100, 28)
    n3 = total - 100 - n2
    parts = [corners, bar((0, 0, 0), 69), _node_lo(o, 1, b1)[None] + [[0.79, 0.39, 0.2]], bar((-1, 0, 0), 30)]
    if n2 == 29:
        # 28 points in the node's first cell, the 29th (last in sorted order: a later cell) just across the face from A's last row
        parts += [bar((1, 0, 0), 28, x=(0.02, 0.38)), _node_lo(o, 1, b1 + (1, 0, 0))[None] + [[0.01, 0.45, 0.2]]]
    else:
        parts.append(bar((1, 0, 0), n2))
    if n3:
        parts.append(bar((0, -1, 0), n3, y=(0.70, 0.79)))
    if p == 'straddle':
        # five more in the +y node, >= 0.41 m from every query: farther than any nearest neighbour (skipped at k = 1), nearer than the
        # 64th neighbour of the lanes at the ends of A (needed at k = 64)
        parts.append(_fill(rng, _node_lo(o, 1, b1 + (0, 1, 0)), 0.3, 0.7, 5))
    return np.concatenate(parts).astype(F32)


def _shell_edge(variant, dim, k):
    """rows: 0, 1 the frame; 2 the query q; then k - 1 near neighbours; row k + 2 = N, the k-th in-shell neighbour, on the -x side; row
    k + 3 = O, the first point beyond the +x outer face of q's level-1 shell.  q sits 1.1 m from that face and >= 1.2 m from the others."""
    rng = np.random.default_rng(5 * k + dim)
    corners, o = _frame()
    b1 = _home(o) + 1
    q = _node_lo(o, 1, b1) + [0.5, 0.4, 0.4]
    near = q + rng.uniform(-0.25, 0.25, size=(k - 1, 3))
    X = _nd(np.concatenate([corners, q[None], near, q[None], q[None]]), dim)
    iq, iN, iO = 2, k + 2, k + 3
    face = _node_lo(o, 1, b1 + 2)[0]                                  # float64 face: a coordinate >= it lies outside the shell
    X[iO, 0] = mr.steps(F32(face + 2e-3), 1)
    X[iN, 1] += F32(0.013)                                            # (N mirrored exactly would TIE with O at some step)
    if variant == 'xyz_in':
        X[iN, 3] = X[iq, 3] + F32(0.3)                                # inside the radius in x,y,z, outside it in dim-D
    P = lambda i: X[i].astype(np.float64)[None]
    extra = lambda i: _d2(P(iq), P(i))[0, 0] - (P(iq)[0, 0] - P(i)[0, 0]) ** 2
    r = face - float(X[iq, 0])                                       # the shell radius of q (asserted against the probe by the aim test)
    if variant == 'in':
        X[iN, 0] = F32(X[iq, 0] - np.sqrt(0.98 * r * r - extra(iN)))
    elif variant == 'xyz_in':
        X[iN, 0] = F32(X[iq, 0] - (r - 0.01))
    else:
        X[iN, 0] = F32(X[iq, 0] - np.sqrt(_d2(P(iq), P(iO))[0, 0] - extra(iN)))
        dN = _d2(P(iq), P(iN))[0, 0]
        x0 = X[iO, 0]
        for s in range(-200, 200):                                    # O's d2 on the two float32-adjacent sides of N's
            X[iO, 0] = mr.steps(x0, s)
            lo_side = _d2(P(iq), P(iO))[0, 0]
            X[iO, 0] = mr.steps(x0, s + 1)
            if lo_side < dN < _d2(P(iq), P(iO))[0, 0]:
                X[iO, 0] = mr.steps(x0, s if variant == 'out_lo' else s + 1)
                break
        else:
            raise AssertionError('no adjacent pair of steps around the k-th distance')
        assert float(X[iO, 0]) >= face
    return X


def _far(case, dim, k):
    """rows 0, 1: the frame; row 2: the lone query q; then the k others.
    A FINITE bound b of phase A satisfies b <= radius(start level) by the choice of the start level, and the level's neighbourhood holds
    the shell, so phase B then ends at the level it starts at and never escalates.  In 3-D b is a distance inside the 2.4 m shell
    (< 2.8 m < any level-3 radius), which reaches the start levels 2 and 3 only; in 4-D the 4th coordinate makes b as large as wanted
    (a dim-D bound against an x,y,z radius), which reaches 4, 5, 6 and the scan of all points.  Only an infinite bound escalates."""
    form, L = case
    half = (80.0, 80.0, 4.0)
    corners, o = _frame(half)
    if form == 'corner':
        corners, _ = _frame((102.3, 102.3, 12.7))
        q = corners[0].astype(np.float64)
        pins = np.stack([corners[1], corners[1] * [1, -1, -1]])      # q itself is the low corner of the bounding box
        return np.concatenate([pins, q[None], _ring(q, 8.0, k, np.radians(5), np.radians(85))]).astype(F32)
    if form == 'clamped':
        q = np.array([300.0, 0.0, 0.0])
        anchors = np.array([[-50.0, -40.0, -4.0], [-50.0, 40.0, 4.0]])
        return np.concatenate([anchors, q[None], _ring(q, 5.0, k, np.radians(100), np.radians(260))]).astype(F32)
    b1 = _home(o)
    if form == 'fin' and L == 3:
        q = _node_lo(o, 1, b1) + 0.05                                 # 1.65 m from the level-2 outer faces, 2.75 m from the shell's far corner
        pts = _ring(q, 1.9, k, np.radians(40), np.radians(50))
    else:
        q = _node_lo(o, 1, b1 + 1) + 0.4
        rad = _radius(np.concatenate([corners, q[None]]), 2)
        mid = lambda l: 0.5 * (rad[l - 1] + rad[l]) if l <= LMAX else rad[LMAX] + 3.0
        if form == 'inf':
            pts = _ring(q, 0.9 * rad[3] if L == 3 else mid(L), k)
        elif form == 'reset':
            j = k // 2
            pts = np.concatenate([_ring(q, 0.9 * rad[3], j), _ring(q, mid(4), k - j, 0.3)])
        elif L == 2:                                                  # in the shell's corners: beyond its radius 1.2, inside the level-2 radius
            quad = [_ring(q, 1.4, (k + 3 - c) // 4, np.radians(90 * c + 33), np.radians(90 * c + 57)) for c in range(min(k, 4))]
            pts = np.concatenate(quad)
        else:
            pts = np.concatenate([_ring(q, 0.3, k), np.full((k, 1), np.sqrt(mid(L) ** 2 - 0.09))], 1)
    assert len(pts) == k
    if pts.shape[1] == 4:
        assert dim == 4
        head = np.concatenate([np.concatenate([corners, q[None]]), np.zeros((3, 1))], 1)
        return np.concatenate([head, pts]).astype(F32)
    return np.concatenate([corners, q[None], pts]).astype(F32)


def _self(case, dim, k):
    """rows 0, 1: the frame; row 2: the query; then c - 1 = k + e copies of it; then 70 points around it"""
    kind, e = case
    rng = np.random.default_rng(9 * k + e)
    corners, o = _frame()
    q = _node_lo(o, 1, _home(o) + 1) + [0.41, 0.43, 0.39]
    around = q + rng.uniform(-0.5, 0.5, size=(70, 3))
    X = _nd(np.concatenate([corners, q[None], np.repeat(q[None], k + e, 0), around]), dim)
    if kind == 'full':
        X[3:3 + k + e] = X[2]
    return X


@functools.lru_cache(maxsize=None)
def scene(family, case, dim, k):
    """-> float32 [n, dim], read-only.  Families whose rows do not depend on k build one array per (case, dim)."""
    if family in ('node_m', 'cell_m', 'shell_cap', 'tile'):
        if k != 0:
            return scene(family, case, dim, 0)
        X = _nd({'node_m': _node_m, 'cell_m': _cell_m, 'shell_cap': _shell_cap, 'tile': _tile}[family](case), dim)
    else:
        X = {'shell_edge': _shell_edge, 'far_L': _far, 'self': _self}[family](case, dim, k)
    X = np.ascontiguousarray(X, F32)
    assert X.shape[1] == dim and np.isfinite(X).all()
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def stage(family, case, dim, k):
    if family in ('node_m', 'cell_m', 'shell_cap', 'tile') and k != 0:
        return stage(family, case, dim, 0)
    return Stage(scene(family, case, dim, k), dim)


@functools.lru_cache(maxsize=None)
def account(family, case, dim, k):
    return stage(family, case, dim, k).run(k)


@functools.lru_cache(maxsize=None)
def expected(family, case, dim, k):
    return core2_dense(scene(family, case, dim, k), k, dim)


def small_scene():
    """n <= k: ten points for k = 15 -- every core distance is +inf"""
    return np.random.default_rng(3).normal(size=(10, 3)).astype(F32), 15
