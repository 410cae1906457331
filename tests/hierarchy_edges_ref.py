"""Generators and restatements of tests/test_hierarchy_edges.py: trees that put the device hierarchy stage (csrc/hdbscan_device.hip) at a
chosen number of true splits, and trees in which ONE cluster's chain has a chosen length and pattern of points per node, with the
excess-of-mass comparison beside it aimed so closely that one wrong chain record flips it.

  switch_constants / switch_points / forms   the LDS switch points of the kernels, read from the source text and restated
  comb                                       a tree with an exact split count
  chain_tree                                 a tree with one chain of a chosen length and kc pattern, aimed by bisection
  restated_difference                        float64 restatement of the stabilities beside the aimed comparison, with single faults
The reference of every comparison is the host stage (csrc/hdbscan_tree.cpp); nothing here runs on a GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_SRC = os.path.join(ROOT, 'vilgod_amd', 'csrc', 'hdbscan_device.hip')


# ---- the switch points, from the source text ---------------------------------------------------------------------------------------------
def switch_constants():
    """-> dict: the three LDS budgets (ints), the threads per workgroup and k_hd_chain_stats' grid size, as hdbscan_device.hip states them"""
    src = open(DEVICE_SRC).read()

    def define(name):
        m = re.search(r'^#define\s+%s\s+(\d+)\b' % name, src, re.M)
        assert m, '%s is no longer a #define with a plain number in hdbscan_device.hip' % name
        return int(m.group(1))

    m = re.search(r'hipLaunchKernelGGL\(\s*k_hd_chain_stats\s*,\s*dim3\((\d+)\)\s*,\s*B\s*,', src)
    assert m, 'the launch of k_hd_chain_stats no longer has a literal grid size and HD_NT threads'
    # the three conditions, as the kernels state them (restated in switch_points below)
    for cond in ('10 * ns <= HD_TREE_LDS_INTS', '3 * ns <= HD_CHAIN_LDS_INTS', '12 * ns + 11 * ncl + 64 <= HD_TREE_BC_LDS_INTS', 'ncl = 2 * ns + 1',
                 'for (int c = 1 + w; c < ncl; c += nw)', 'w == nw - 1'):
        assert cond in src, 'hdbscan_device.hip no longer states `%s`: restate the condition in hierarchy_edges_ref.py and move the cases' % cond
    return dict(tree_a=define('HD_TREE_LDS_INTS'), chain=define('HD_CHAIN_LDS_INTS'), tree_bc=define('HD_TREE_BC_LDS_INTS'), nt=define('HD_NT'),
                stats_grid=int(m.group(1)))


def forms(ns, k):
    """-> the form of each kernel at `ns` true splits: (k_hd_tree_a, k_hd_chain, k_hd_tree_bc, last wave of k_hd_chain_stats owns a cluster,
    the bitonic sort's padded length)"""
    ncl = 2 * ns + 1
    waves = k['stats_grid'] * (k['nt'] // 64)
    p = 1
    while p < ns:
        p <<= 1
    return ('lds' if 10 * ns <= k['tree_a'] else 'global', 'lds' if 3 * ns <= k['chain'] else 'global',
            'lds' if 12 * ns + 11 * ncl + 64 <= k['tree_bc'] else 'global', 1 + (waves - 1) < ncl, p)


def switch_points(k):
    """-> (last ns of k_hd_tree_bc in LDS, of k_hd_tree_a, of k_hd_chain, first ns at which the last wave of k_hd_chain_stats owns a cluster)"""
    last = lambda i: max(ns for ns in range(1, 20000) if forms(ns, k)[i] == 'lds')
    return last(2), last(0), last(1), min(ns for ns in range(1, 20000) if forms(ns, k)[3])


def describe(ns_values, k):
    return '; '.join('ns %d: tree_a %s, chain %s, tree_bc %s, last stats wave %s, sort pad %d'
                     % ((ns,) + forms(ns, k)[:3] + ('owns a cluster' if forms(ns, k)[3] else 'root only', forms(ns, k)[4])) for ns in ns_values)


# ---- the emulation with its sweep count --------------------------------------------------------------------------------------------------
def emul_tree_sweeps(lib, lo, hi, w2, n, mcs, opt):
    """tests/emul/hdbscan_select_emul.cpp -> (labels, probs, n_clusters, ns, sweeps)"""
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    labels, probs = np.empty(n, np.int32), np.empty(n, np.float64)
    nc, ns, sw = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.hd_emul_tree_ex(p(lo), p(hi), p(w2), n, mcs, ctypes.c_double(opt[2]), 1 if opt[0] == 'leaf' else 0, int(opt[1]), int(opt[3]), p(labels),
                             p(probs), ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(sw))
    assert rc == 0, rc
    return labels, probs, nc.value, ns.value, sw.value


def _finish(rng, n, u, v, w):
    """permute the vertices, sort by w2 ONLY (ties shuffled), as tests/test_hierarchy.py's random_tree does -> (lo, hi, w2, perm)"""
    perm = rng.permutation(n)
    a, b = perm[np.asarray(u)], perm[np.asarray(v)]
    l2, h2 = np.minimum(a, b).astype(np.int32), np.maximum(a, b).astype(np.int32)
    w = np.asarray(w, np.float64)
    w2 = w * w
    sh = rng.permutation(len(w2))
    order = sh[np.argsort(w2[sh], kind='stable')]
    return np.ascontiguousarray(l2[order]), np.ascontiguousarray(h2[order]), np.ascontiguousarray(w2[order]), perm


# ---- A: an exact split count -------------------------------------------------------------------------------------------------------------
def comb(rng, S, mcs, shape, extra, mode='light', tail=0, tail_scale=None):
    """-> (lo, hi, w2, n, group [n]): S + 1 groups of mcs .. mcs + extra points, a random tree inside each, S joining edges between groups;
    tail > 0: that many nodes of a chain of the ROOT's besides (group S + 1), which k_hd_chain_stats walks under allow_single_cluster.

    A join is a true split iff, at its rank, both endpoints reach >= mcs vertices over lighter edges; a group has fewer than 2 mcs points
    (extra < mcs), so with every inner edge of a group lighter than every join that touches the group, each join has a whole group on both
    sides and no inner edge has mcs points on both: ns == S.  A group of exactly mcs points leaves no other choice -- one inner edge at or
    above a touching join and that join is no split -- so that is the rule of both weight modes, and no group ever has to be redrawn:
      light   inner weights 10 .. 100 times below the lightest join: the leaves always win the excess of mass;
      mixed   a group's inner weights between 0.5 and 1.0 times the weight of its own join (group 0: of its lightest join), capped
              below the lightest join that touches the group; the joins' weights keep every child's join above half its parent's, so
              the interval is never empty.  The two groups at the lightest join get inner weights just under it and a parent born at
              least 6 % above it, so that one parent beats its two leaves by construction; elsewhere parents and leaves both win.
    shape: spine (g joins g - 1, weights rising), balanced (g joins (g - 1) // 2, weight falling with the level), random (a random
    earlier group, weights a random factor of the parent's)."""
    assert 0 <= extra < mcs and S >= 1
    G = S + 1
    size = mcs + (rng.integers(0, extra + 1, G) if extra else np.zeros(G, np.int64))
    off = np.concatenate(([0], np.cumsum(size)))
    n = int(off[-1])
    g = np.arange(1, G)
    W = np.zeros(G)                                                 # W[g]: weight of group g's own join (g >= 1)
    if shape == 'spine':
        par = g - 1
        W[1:] = 0.05 * (1.0 + np.cumsum(rng.uniform(0.0, 0.5, S) * (rng.random(S) < 0.3)) + 0.05 * g)
    elif shape == 'balanced':
        par = (g - 1) // 2
        level = np.floor(np.log2(g + 1)).astype(np.int64)          # groups 1, 2: level 1
        W[1:] = 0.4 * 0.9 ** (level - 1) * rng.uniform(0.95, 1.0, S)
    else:
        assert shape == 'random'
        par = (rng.random(S) * g).astype(np.int64)
        W[0] = 0.15
        f = rng.uniform(0.7, 1.5, S)
        for i in range(S):                                          # (parents come first)
            W[i + 1] = min(max(W[par[i]] * f[i], 0.01), 20.0) if par[i] else 0.15 * f[i]
        W[0] = 0.0
    assert len(np.unique(W[1:])) == S
    jmin = 1 + int(np.argmin(W[1:]))                                # the lightest join: a single group on both sides, two leaves under one parent
    if mode == 'mixed' and S > 1:
        # ... and that parent is made to win: its birth (the next join that touches the pair) at least 6 % above its split in weight,
        # the two leaves' inner weights (below) within 0.5 % under the split
        pair = (jmin, par[jmin - 1])
        others = [W[j] for j in range(1, G) if j != jmin and (j in pair or par[j - 1] in pair)]
        W[jmin] = min(W[jmin], min(others) / 1.06)
    touch = np.full(G, np.inf)                                      # the lightest join that touches the group
    np.minimum.at(touch, g, W[1:])
    np.minimum.at(touch, par, W[1:])
    vg = np.repeat(np.arange(G), size)                              # group of every vertex
    local = np.arange(n) - off[vg]
    inner = local > 0
    iu = np.arange(n)[inner]
    iv = off[vg[inner]] + (rng.random(inner.sum()) * local[inner]).astype(np.int64)    # a random earlier vertex of the same group
    ig = vg[inner]
    if mode == 'light':
        iw = W[1:].min() * rng.uniform(0.01, 0.1, len(iu))
    else:
        assert mode == 'mixed'
        own = np.where(np.arange(G) == 0, touch, W)
        assert (touch > 0.5 * own).all()
        hi_w = np.minimum(own, touch)
        iw = 0.5 * own[ig] + rng.random(len(iu)) * (0.999 * hi_w[ig] - 0.5 * own[ig])
        if S > 1:
            weak = (ig == jmin) | (ig == par[jmin - 1])
            iw[weak] = W[jmin] * rng.uniform(0.995, 0.999, int(weak.sum()))
        assert (iw >= 0.5 * own[ig]).all() and (iw < own[ig]).all()
    assert (iw < touch[ig]).all()
    ju = off[g] + (rng.random(S) * size[g]).astype(np.int64)
    jv = off[par] + (rng.random(S) * size[par]).astype(np.int64)
    u, v, w = [iu, ju], [iv, jv], [iw, W[1:]]
    if tail:
        # the root's own chain: a path hung on a random vertex, every edge heavier than every join and rising outwards (one node of the
        # root's chain each, never a split); every seventh node carries a second point on a far lighter edge (kc = 2)
        assert mcs >= 3
        twigs = np.arange(tail)[::7]
        path = n + np.arange(tail)
        rise = 1.5 + 0.01 * np.arange(tail) if tail_scale is None else 1.001 + tail_scale * (1.0 + np.arange(tail)) / tail
        u.append(path); v.append(np.concatenate(([rng.integers(0, n)], path[:-1]))); w.append(W[1:].max() * rise)
        u.append(n + tail + np.arange(len(twigs))); v.append(path[twigs]); w.append(W[1:].min() * rng.uniform(1e-4, 1e-3, len(twigs)))
        vg = np.concatenate((vg, np.full(tail + len(twigs), G)))
        n += tail + len(twigs)
    lo, hi, w2, perm = _finish(rng, n, np.concatenate(u), np.concatenate(v), np.concatenate(w))
    group = np.empty(n, np.int64)
    group[perm] = vg
    return lo, hi, w2, n, group


def selected_kinds(labels, group):
    """-> (selected clusters that are one whole group = leaves of a comb tree, selected clusters that span several groups)"""
    leaves = parents = 0
    for lab in np.unique(labels[labels >= 0]):
        if len(np.unique(group[labels == lab])) == 1:
            leaves += 1
        else:
            parents += 1
    return leaves, parents


# ---- B: one chain of a chosen length and kc pattern --------------------------------------------------------------------------------------
PATTERNS = ('ones', 'first', 'lane63', 'middle', 'tail', 'all')
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
WHICH = ('parent', 'leaf', 'root')


def kc_pattern(L, pattern, mcs):
    """-> kc of the L designed chain nodes by POSITION in the wave's order (0 = the highest rank = lane 0 of the first 64-record step).
    One node of mcs - 1 points: first = lane 0 of the first step; lane63 = the lowest rank of the first step (of the only step when it is
    short); middle = lane 31 of the first step, the rest of the step one point each; tail = the lowest rank of the last step."""
    kc = np.ones(L, np.int64)
    if pattern == 'all':
        kc = 2 + np.arange(L) % (mcs - 2)                           # 2 .. mcs - 1
    elif pattern != 'ones':
        kc[{'first': 0, 'lane63': min(63, L - 1), 'middle': min(31, L // 2), 'tail': L - 1}[pattern]] = mcs - 1
    return kc


class _Builder:
    def __init__(self):
        self.n, self.u, self.v, self.w = 0, [], [], []

    def vertex(self):
        self.n += 1
        return self.n - 1

    def edge(self, u, v, w):
        self.u.append(u); self.v.append(v); self.w.append(w)
        return len(self.w) - 1

    def blob(self, mcs, w_top, rng):
        """a path of exactly mcs points, its heaviest edge w_top: a leaf's last chain node -- both sides below mcs, all mcs points leave
        there.  -> (a vertex of it, the record (w_top, mcs))"""
        vs = [self.vertex() for _ in range(mcs)]
        for i in range(1, mcs):
            self.edge(vs[i - 1], vs[i], w_top if i == mcs - 1 else w_top * rng.uniform(0.1, 0.5))
        return vs[0], (w_top, mcs)

    def chain(self, at, weights, kc, rng):
        """a path hung on vertex `at`, weights rising outwards: cutting the heaviest remaining edge takes the outermost node off; a node
        of kc points = the path vertex and a twig of kc - 1 points on far lighter edges.  weights / kc by POSITION (0 = outermost = the
        highest rank).  -> the records [(w, kc)] by position"""
        prev = at
        for w, k in list(zip(weights, kc))[::-1]:                   # innermost first
            q = self.vertex()
            self.edge(prev, q, w)
            for _ in range(int(k) - 1):
                self.edge(q, self.vertex(), w * 1e-4 * rng.uniform(0.1, 1.0))
            prev = q
        return [(float(w), int(k)) for w, k in zip(weights, kc)]


def _lam(w):
    w = np.asarray(w, np.float64)
    return 1.0 / np.sqrt(w * w)                                     # (the tree carries w2; hd_lambda: 1 / sqrt(w2))


def _chain_sum(records, birth, fault=None):
    """hd_chain_stats: the chain's rows by descending rank, kc equal terms each, added one after the other.  fault: ('drop', i),
    ('double', i), ('one', i) = node i counted as one point, ('extra', (w, kc)) = a record from outside the run taken in"""
    recs = list(records)
    if fault and fault[0] == 'extra':
        recs.append(fault[1])
    if not recs:
        return 0.0
    t = (_lam(np.array([w for w, _ in recs], np.float64)) - birth) * 1.0
    reps = np.array([kc for _, kc in recs], np.int64)
    if fault and fault[0] != 'extra':
        reps[fault[1]] = {'drop': 0, 'double': 2 * reps[fault[1]], 'one': 1}[fault[0]]
    terms = np.repeat(t, reps)
    return float(np.cumsum(terms)[-1]) if len(terms) else 0.0      # (cumsum adds one after the other, in order)


def restated_difference(d, split_w, fault=None):
    """-> stability(parent) - (stability(kid 0) + stability(kid 1)) beside the aimed comparison, the way hd_chain_stats and hd_up_node /
    hd_root_node state them: the parent's own chain, then its two child rows (lambda of its split - birth) * size, side 0 first; the kids
    are leaves: their chains alone.  `fault` applies to the chain under test.  The parent wins iff the difference is >= 0."""
    birth = _lam(d['birth_w']) if d['birth_w'] else 0.0
    lam_s = _lam(split_w)
    under = d['under']                                              # 'parent', 0 or 1 (the kid whose chain it is)
    s = _chain_sum(d['parent_records'], birth, fault if under == 'parent' else None)
    for k in (0, 1):
        s += (lam_s - birth) * float(d['kid_size'][k])
    sub = 0.0
    for k in (0, 1):
        sub += _chain_sum(d['kid_records'][k], lam_s, fault if under == k else None)
    return s - sub


def smallest_term(d, split_w):
    birth = (_lam(d['birth_w']) if d['birth_w'] else 0.0) if d['under'] == 'parent' else _lam(split_w)
    recs = d['parent_records'] if d['under'] == 'parent' else d['kid_records'][d['under']]
    return min(_lam(w) - birth for w, _ in recs)


def chain_tree(L, pattern, which, mcs, aim, seed=0):
    """-> dict(lo, hi, w2, n, opt, d, split_w, margin, tmin, a1, a2, outside): a tree in which ONE cluster has a chain of exactly L nodes.

    which = 'parent': cluster A (two child clusters A1, A2, a sibling B under the root) has the chain, every node as `pattern` says;
            'leaf':   A1 has it.  A leaf's last node (the lowest rank) always holds the mcs points that are left, so the pattern describes
                      the other L - 1 nodes, and A has no chain of its own;
            'root':   the root has it, under allow_single_cluster; its children are R1, R2 and there is no B.
    The children's inner edges are light (their points leave at large lambdas), so the difference parent - children rises steadily from
    negative to positive as the weight of the parent's split falls through its allowed interval; `aim` = +1: bisected to the weight at which
    the parent wins by half the smallest single term (lambda - birth) of the chain under test, -1: at which the children win by that much.
    `a1`, `a2`: a point of each child (the same label iff the parent is selected).  `outside`: the records just outside the chain's run in
    the device's sorted chain array (the highest rank of the run before, the lowest rank of the run after), where there is one."""
    rng = np.random.default_rng([seed, L, PATTERNS.index(pattern), WHICH.index(which), mcs, aim + 1])
    b = _Builder()
    if which == 'leaf':
        # lambdas: the chain 50 .. 80, what is left of A1 90, A2 95; the split of A anywhere below 50
        kc = kc_pattern(L - 1, pattern, mcs) if L > 1 else np.zeros(0, np.int64)
        a1, last = b.blob(mcs, 1.0 / 90.0, rng)
        recs1 = b.chain(a1, np.linspace(1.0 / 50.0, 1.0 / 80.0, L - 1), kc, rng) + [last]
        a2, last2 = b.blob(mcs, 1.0 / 95.0, rng)
        recs = [recs1, [last2]]
        parent_records = []
        w_lo, w_hi = (1.0 / 50.0) * 1.02, 4.0 * 0.98
    else:
        # lambdas: the chain 0.5 .. 1, the children 1000 and 1100; the split anywhere between
        kc = kc_pattern(L, pattern, mcs)
        a1, last1 = b.blob(mcs, 1.0 / 1000.0, rng)
        a2, last2 = b.blob(mcs, 1.0 / 1100.0, rng)
        recs = [[last1], [last2]]
        parent_records = b.chain(a1, np.linspace(2.0, 1.0, L), kc, rng)
        w_lo, w_hi = (1.0 / 1000.0) * 1.02, 1.0 * 0.98
    e_split = b.edge(a1, a2, 0.0)                                   # (its weight: below)
    if which != 'root':
        vb, last_b = b.blob(mcs, 1.0 / 1200.0, rng)
        b.edge(a1, vb, 4.0)
    kid_n = [sum(k for _, k in r) for r in recs]
    # which side of the split is side 0 (the `lo` endpoint's) is known only once the vertices are permuted: draw the permutation first
    perm = rng.permutation(b.n)
    first = 0 if perm[a1] < perm[a2] else 1                         # the kid on side 0
    d = dict(birth_w=None if which == 'root' else 4.0, parent_records=parent_records,
             kid_records=[recs[first], recs[1 - first]], kid_size=[kid_n[first], kid_n[1 - first]],
             under='parent' if which != 'leaf' else (0 if first == 0 else 1))
    target = lambda w: restated_difference(d, w) - aim * 0.5 * smallest_term(d, w)
    assert target(w_hi) < 0.0 < target(w_lo), 'the case cannot be aimed: %r' % ((L, pattern, which, mcs, aim),)
    lo_w, hi_w = w_lo, w_hi                                         # the difference falls as the weight rises
    for _ in range(80):
        mid = 0.5 * (lo_w + hi_w)
        if target(mid) > 0.0:
            lo_w = mid
        else:
            hi_w = mid
    split_w = lo_w if aim > 0 else hi_w
    b.w[e_split] = split_w
    u, v, w = perm[np.asarray(b.u)], perm[np.asarray(b.v)], np.asarray(b.w, np.float64)
    w2 = w * w
    assert len(np.unique(w2)) == len(w2)                            # no ties: the ranks are the weights' order
    order = np.argsort(w2, kind='stable')
    lo, hi = np.minimum(u, v).astype(np.int32)[order], np.maximum(u, v).astype(np.int32)[order]
    # the runs of the sorted chain array: provisional ids 1 + 2 k + side by split rank k, then the root's run
    if which == 'root':
        runs = [('kid', 0), ('kid', 1), ('parent',)]
    else:
        b_first = perm[vb] < perm[a1]                               # the root split: B on side 0?
        runs = [('kid', 0), ('kid', 1)] + ([('b',), ('parent',)] if b_first else [('parent',), ('b',)])
    run_recs = {('kid', 0): d['kid_records'][0], ('kid', 1): d['kid_records'][1], ('parent',): parent_records}
    if which != 'root':
        run_recs[('b',)] = [last_b]
    runs = [r for r in runs if run_recs[r]]
    at = runs.index(('parent',) if d['under'] == 'parent' else ('kid', d['under']))
    outside = []
    if at > 0:
        outside.append(run_recs[runs[at - 1]][0])                   # position 0: the highest rank of the run before
    if at + 1 < len(runs):
        outside.append(run_recs[runs[at + 1]][-1])                  # the lowest rank of the run after
    return dict(lo=np.ascontiguousarray(lo), hi=np.ascontiguousarray(hi), w2=np.ascontiguousarray(w2[order]), n=b.n,
                opt=('eom', which == 'root', 0.0, 0), d=d, split_w=split_w, tmin=smallest_term(d, split_w),
                margin=restated_difference(d, split_w), a1=int(perm[a1]), a2=int(perm[a2]), outside=outside, n_other=0 if which == 'root' else 1)


def chain_cases():
    for which in WHICH:
        for mcs in (5, 15):
            for L in LENGTHS:
                for pattern in PATTERNS:
                    for aim in (1, -1):
                        yield which, mcs, L, pattern, aim
