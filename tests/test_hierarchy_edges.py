"""The device hierarchy stage (csrc/hdbscan_device.hip) at the split counts where its kernels change form, and at the steps of
k_hd_chain_stats' wave walk -- against the host stage (csrc/hdbscan_tree.cpp) on the same tree: cluster count equal, labels equal,
probabilities equal as uint64.  Generators and restatements: tests/hierarchy_edges_ref.py.

A  "comb" trees with an exact number of true splits ns, on both sides of every switch: k_hd_tree_bc in LDS up to ns 1142, k_hd_tree_a
   (Kruskal) up to 3072, k_hd_chain up to 4096, the last wave of k_hd_chain_stats owning a cluster from 1024, the bitonic sort's padding at
   1024 / 2048 / 4096 -- the switch points derived from the constants in the source text, not typed in.  One handle across the forms, and the
   same calls on one stream with nothing waited for in between.
B  trees in which ONE cluster's chain has a chosen length (1 .. 200: below, at and above one and two 64-record steps) and pattern of points
   per node, the excess-of-mass comparison beside it aimed by bisection to a quarter .. three quarters of the chain's smallest single term: a
   dropped or doubled record, a node of several points taken as one, or the record just outside the run taken in flips the selection (shown in
   a float64 restatement on the CPU).  What these cases CANNOT see: a sum that has the right terms in another order, which moves only the last
   bits of a stability and no selection; and a record lost from a LEAF's sum and point count at once, which takes about as much from the
   parent's child row as from the leaf (the parent's and the root's chains see that one).  The chain's `death` and `npts` show in the
   probabilities and the cluster sizes, as everywhere.
   A comb tree with a long chain of the root's, scaled to where the root's win under allow_single_cluster turns into a loss, does the same
   for the root's chain at the split counts from which the wave that walks it owns a cluster too.
CPU: the generators' guarantees, the emulation of the device rules and the host stage on these trees (and the host stage against scikit-learn
on the comb family).  GPU: the kernels."""
import numpy as np
import pytest

import hierarchy_edges_ref as R
from test_hdbscan_selection import emul  # noqa: F401  (the emulation, built once per module)
from test_hdbscan_selection import EOM, EOM_MAX200, EOM_SINGLE, LEAF, OPTION_SETS, device_tree_ex, host_tree_ex

SHAPES = ('spine', 'balanced', 'random')
MODES = ('light', 'mixed')
SPLITS = (1, 2, 1023, 1024, 1025, 1142, 1143, 2048, 2049, 3072, 3073, 4096, 4097)
EXTRA = {2: 0, 3: 2, 15: 0, 32: 0}                                  # min_cluster_size -> up to that many more points per group


def same(a, b):
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def comb_sizes(S):
    return (2, 3, 15, 32) if S in (1142, 1143) else (2, 3)


def comb_options(S):
    """every entry of OPTION_SETS (its own epsilon aside) at epsilon 0 and 0.15 up to 1143 splits; four of them above"""
    sets = OPTION_SETS if S <= 1143 else (EOM, LEAF, EOM_SINGLE, EOM_MAX200)
    out = []
    for method, single, _, max_size in sets:
        for eps in (0.0, 0.15):
            if (method, single, eps, max_size) not in out:
                out.append((method, single, eps, max_size))
    return out


def comb_tree(S, shape, mode, mcs, seed=0):
    """min_cluster_size 2: nothing but the groups, the densest tree; 3: a chain of the root's of 70 nodes (more than one 64-record step)
    besides, so that the wave that walks the root's chain has one to walk on both sides of the split count from which it owns clusters too"""
    rng = np.random.default_rng([seed, S, SHAPES.index(shape), MODES.index(mode), mcs])
    return R.comb(rng, S, mcs, shape, EXTRA[mcs], mode, tail=70 if mcs == 3 else 0)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_switch_points_are_where_the_cases_are():
    """the cases of this module sit on both sides of every switch of hdbscan_device.hip; whoever changes a constant there moves them"""
    k = R.switch_constants()
    points = R.switch_points(k)
    assert points == (1142, 3072, 4096, 1024), 'the kernels of hdbscan_device.hip change form at other split counts now (%r): move SPLITS' % (points,)
    for last in points[:3]:
        assert last in SPLITS and last + 1 in SPLITS
    assert points[3] - 1 in SPLITS and points[3] in SPLITS
    for p in (1024, 2048, 4096):                                    # the bitonic sort's padding
        assert R.forms(p, k)[4] == p and R.forms(p + 1, k)[4] == 2 * p and p in SPLITS and p + 1 in SPLITS
    assert R.forms(3073, k)[:3] == ('global', 'lds', 'global') and R.forms(4097, k)[:3] == ('global', 'global', 'global')
    assert R.forms(1143, k)[:3] == ('lds', 'lds', 'global') and R.forms(1142, k)[:3] == ('lds', 'lds', 'lds')


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('S', SPLITS)
def test_comb_rules_equal_the_host_stage_at_the_exact_split_count(emul, S, shape):
    for mode in MODES:
        for mcs in comb_sizes(S):
            lo, hi, w2, n, group = comb_tree(S, shape, mode, mcs)
            for opt in comb_options(S):
                want = host_tree_ex(lo, hi, w2, n, mcs, opt)
                L, P, c, ns, _ = R.emul_tree_sweeps(emul, lo, hi, w2, n, mcs, opt)
                assert ns == S, (mode, mcs, opt)
                assert same(want, (L, P, c)), (mode, mcs, opt)
                if opt == EOM:
                    leaves, parents = R.selected_kinds(want[0], group)
                    assert leaves >= 1, (mode, mcs)
                    if mode == 'mixed' and S > 1:                   # (one split: the root's two children are the only clusters)
                        assert parents >= 1, (mode, mcs)
                    if mode == 'light':
                        assert parents == 0 and leaves == S + 1


# The root's chain where the wave that walks it also owns a cluster (from 1024 splits on): a comb tree with a chain of the root's so long that
# the root wins the excess of mass under allow_single_cluster, its weights scaled by bisection ON THE HOST STAGE to the two neighbouring
# scales between which the root's win turns into a loss.  There the comparison root-against-children is decided in the last bits: a record
# of the root's chain lost shows in the first tree, one too many in the second, and so may even the right terms in another order.
ROOT_EDGE = [(1023, 'spine', 2000), (1024, 'spine', 2000), (1143, 'spine', 2000), (1023, 'random', 8000), (1024, 'random', 8000)]


def root_edge_trees(S, shape, tail):
    """-> (tree in which the root barely wins, tree in which it barely loses, relative distance of the two scales)"""
    def tree(scale):
        rng = np.random.default_rng([7, S, SHAPES.index(shape)])
        return R.comb(rng, S, 3, shape, EXTRA[3], 'mixed', tail=tail, tail_scale=scale)

    def root_wins(t):
        labels, _, c = host_tree_ex(t[0], t[1], t[2], t[3], 3, EOM_SINGLE)
        return c == 1 and (labels == 0).any()                      # (so many splits: one cluster can only be the root)

    lo_s, hi_s = 1e-9, 1e3                                          # (the chain's weights rise with the scale: its lambdas fall)
    win, lose = tree(lo_s), tree(hi_s)
    assert root_wins(win) and not root_wins(lose), 'the root cannot be aimed on this tree: %r' % ((S, shape, tail),)
    for _ in range(120):
        mid = (lo_s * hi_s) ** 0.5
        if not lo_s < mid < hi_s:
            break
        t = tree(mid)
        if root_wins(t):
            lo_s, win = mid, t
        else:
            hi_s, lose = mid, t
    return win, lose, hi_s / lo_s - 1.0


@pytest.mark.parametrize('S,shape,tail', ROOT_EDGE)
def test_root_chain_rules_at_the_turn_of_the_excess_of_mass(emul, S, shape, tail):
    win, lose, gap = root_edge_trees(S, shape, tail)
    assert gap < 1e-12                                              # neighbouring scales: the two trees differ in the chain's last bits
    for lo, hi, w2, n, _ in (win, lose):
        want = host_tree_ex(lo, hi, w2, n, 3, EOM_SINGLE)
        L, P, c, ns, _ = R.emul_tree_sweeps(emul, lo, hi, w2, n, 3, EOM_SINGLE)
        assert ns == S and same(want, (L, P, c))
    assert host_tree_ex(*win[:4], 3, EOM_SINGLE)[2] == 1 and host_tree_ex(*lose[:4], 3, EOM_SINGLE)[2] > 1


@pytest.mark.parametrize('S', (7, 64, 300))
def test_host_stage_equals_scikit_learn_on_comb_trees(S):
    """the reference of this module against ITS reference, as test_hdbscan_selection.test_host_stage_equals_scikit_learn does"""
    import hdbscan_select_ref as ref
    from oracle import hdbscan_oracle as ho
    for shape in SHAPES:
        for mode in MODES:
            for mcs in (2, 3, 15):
                lo, hi, w2, n, _ = comb_tree(S, shape, mode, mcs)
                for opt in OPTION_SETS:
                    want_l, want_p = ref.tree_to_labels(lo, hi, w2, mcs, *opt)
                    got_l, got_p, nc = host_tree_ex(lo, hi, w2, n, mcs, opt)
                    assert np.array_equal(got_l < 0, want_l < 0), (shape, mode, mcs, opt)
                    assert np.array_equal(ho.canonical(got_l), ho.canonical(want_l)), (shape, mode, mcs, opt)
                    assert float(np.abs(got_p - want_p).max()) <= 1e-9, (shape, mode, mcs, opt)
                    if nc != len(set(want_l[want_l >= 0].tolist())):
                        assert opt[1] and nc == 1 and (want_l < 0).all(), (shape, mode, mcs, opt)


def chain_ids(which, mcs):
    return [(m, L) for w, m, L, pattern, aim in R.chain_cases() if w == which and m == mcs and pattern == 'ones' and aim == 1]


def chain_batch(which, mcs, L):
    return [(pattern, aim, R.chain_tree(L, pattern, which, mcs, aim)) for pattern in R.PATTERNS for aim in (1, -1)]


def selects_parent(c, labels):
    return labels[c['a1']] >= 0 and labels[c['a1']] == labels[c['a2']]


@pytest.mark.parametrize('mcs', (5, 15))
@pytest.mark.parametrize('which', R.WHICH)
def test_chain_cases_are_aimed_and_see_their_faults(emul, which, mcs):
    """every case: the host stage selects as aimed, the restated margin is a quarter .. three quarters of the chain's smallest single term,
    and in the restatement each single fault flips the comparison under the aim it suits -- a fault that takes from the chain's cluster under
    the aim that cluster wins, one that adds to it under the other.  The emulation equals the host stage."""
    seen = set()
    for mcs, L in chain_ids(which, mcs):
        for pattern, aim, c in chain_batch(which, mcs, L):
            key = (mcs, L, pattern, aim)
            d, w = c['d'], c['split_w']
            assert c['margin'] == R.restated_difference(d, w) and (c['margin'] >= 0) == (aim > 0), key
            assert 0.25 * c['tmin'] <= abs(c['margin']) <= 0.75 * c['tmin'], key
            want = host_tree_ex(c['lo'], c['hi'], c['w2'], c['n'], mcs, c['opt'])
            assert selects_parent(c, want[0]) == (aim > 0), key
            assert want[2] == c['n_other'] + (1 if aim > 0 else 2), key
            L1, P1, c1, ns, _ = R.emul_tree_sweeps(emul, c['lo'], c['hi'], c['w2'], c['n'], mcs, c['opt'])
            assert ns == (1 if which == 'root' else 2) and same(want, (L1, P1, c1)), key
            recs = d['parent_records'] if d['under'] == 'parent' else d['kid_records'][d['under']]
            assert len(recs) == L, key
            # the chain's cluster wins under this aim: faults that TAKE from it flip; it loses: faults that ADD to it flip
            chain_wins = (aim > 0) == (d['under'] == 'parent')
            flips = lambda fault: (R.restated_difference(d, w, fault) >= 0) != (aim > 0)
            for i, (_, kc) in enumerate(recs):
                if chain_wins:
                    assert flips(('drop', i)), (key, i)
                    if kc > 1:
                        assert flips(('one', i)), (key, i)
                        seen.add('one')
                else:
                    assert flips(('double', i)), (key, i)
            if not chain_wins:
                assert c['outside'], key
                for rec in c['outside']:
                    assert flips(('extra', rec)), (key, rec)
                seen.add('extra')
            seen.add('drop' if chain_wins else 'double')
    assert seen == {'drop', 'double', 'one', 'extra'}


def test_chain_patterns_sit_on_the_step_edges():
    """the pattern positions in the wave's order: lane 0, lane 63 and lane 31 of the first full step, the lowest rank of the tail step"""
    for L in R.LENGTHS:
        for mcs in (5, 15):
            assert (R.kc_pattern(L, 'ones', mcs) == 1).all()
            assert ((R.kc_pattern(L, 'all', mcs) >= 2) & (R.kc_pattern(L, 'all', mcs) < mcs)).all()
            for pattern, at in (('first', 0), ('lane63', min(63, L - 1)), ('middle', min(31, L // 2)), ('tail', L - 1)):
                kc = R.kc_pattern(L, pattern, mcs)
                assert kc[at] == mcs - 1 and kc.sum() == L + mcs - 2
    assert {L % 64 for L in R.LENGTHS} >= {0, 1, 63} and max(R.LENGTHS) > 128


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('S', SPLITS)
def test_device_stage_at_the_exact_split_count(cuda, emul, S, shape, mode):
    """a handle of exactly the tree's size: with min_cluster_size 2 and no extra point, the densest split count such a handle can meet"""
    from vilgod_amd.hdbscan import DeviceHierarchy
    k = R.switch_constants()
    sweeps = []
    for mcs in comb_sizes(S):
        lo, hi, w2, n, _ = comb_tree(S, shape, mode, mcs)
        ns, sw = R.emul_tree_sweeps(emul, lo, hi, w2, n, mcs, EOM)[3:]
        assert ns == S
        sweeps.append(sw)
        h = DeviceHierarchy(max_points=n, device=cuda)
        for opt in comb_options(S):
            want = host_tree_ex(lo, hi, w2, n, mcs, opt)
            assert same(want, device_tree_ex(h, cuda, lo, hi, w2, n, mcs, opt)), (mcs, opt)
    print('\ncomb %s %s: %s; emulation sweeps %s' % (shape, mode, R.describe([S], k), sweeps))


CROSS = (4097, 300, 3073, 1143, 1142, 3072, 4096, 1, 4097)


def cross_trees(shape):
    trees = {S: comb_tree(S, shape, 'mixed', 2) for S in set(CROSS)}
    again = comb_tree(4097, shape, 'mixed', 2, seed=1)             # (the second visit of 4097: another tree)
    return [trees[S] for S in CROSS[:-1]] + [again]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_one_handle_across_the_forms(cuda, shape):
    """a call in one form must not read what a call in another form left in the handle's slab"""
    from vilgod_amd.hdbscan import DeviceHierarchy
    opt = ('eom', True, 0.15, 0)
    h = DeviceHierarchy(max_points=17_000, device=cuda)
    for S, (lo, hi, w2, n, _) in zip(CROSS, cross_trees(shape)):
        want = host_tree_ex(lo, hi, w2, n, 2, opt)
        assert same(want, device_tree_ex(h, cuda, lo, hi, w2, n, 2, opt)), S
        assert same(want, device_tree_ex(DeviceHierarchy(max_points=n, device=cuda), cuda, lo, hi, w2, n, 2, opt)), S
    print('\none handle, %s: %s' % (shape, R.describe(CROSS, R.switch_constants())))


@pytest.mark.gpu
def test_the_forms_in_a_row_on_one_stream_without_a_host_read(cuda):
    """the sequence twice, every call queued behind the other on one stream, its own output buffers, nothing waited for until the end"""
    import torch
    from vilgod_amd.hdbscan import DeviceHierarchy
    opt = ('eom', True, 0.15, 0)
    trees = cross_trees('random')
    want = [host_tree_ex(lo, hi, w2, n, 2, opt) for lo, hi, w2, n, _ in trees]
    dev = [[torch.from_numpy(a).to(cuda) for a in t[:3]] for t in trees]
    h = DeviceHierarchy(max_points=17_000, device=cuda)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=cuda)
    got = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            for (lo, hi, w2), t in zip(dev, trees):
                got.append(h.tree_async(lo, hi, w2, t[3], 2, opt[2], stream, 0, 1, 0))
    stream.synchronize()
    for i, (labels, probs, nc) in enumerate(got):
        assert same(want[i % len(trees)], (labels.cpu().numpy(), probs.cpu().numpy(), int(nc.item()))), i


@pytest.mark.gpu
@pytest.mark.parametrize('S,shape,tail', ROOT_EDGE)
def test_device_stage_on_the_root_chain_at_the_turn_of_the_excess_of_mass(cuda, S, shape, tail):
    from vilgod_amd.hdbscan import DeviceHierarchy
    win, lose, gap = root_edge_trees(S, shape, tail)
    counts = []
    for lo, hi, w2, n, _ in (win, lose):
        want = host_tree_ex(lo, hi, w2, n, 3, EOM_SINGLE)
        assert same(want, device_tree_ex(DeviceHierarchy(max_points=n, device=cuda), cuda, lo, hi, w2, n, 3, EOM_SINGLE))
        counts.append(want[2])
    assert counts[0] == 1 and counts[1] > 1
    print('\nroot chain of %d nodes, %s: %s; clusters %s at scales %.1e apart' % (tail, shape, R.describe([S], R.switch_constants()), counts, gap))


@pytest.mark.gpu
@pytest.mark.parametrize('mcs', (5, 15))
@pytest.mark.parametrize('which', R.WHICH)
def test_device_stage_on_the_aimed_chains(cuda, emul, which, mcs):
    from vilgod_amd.hdbscan import DeviceHierarchy
    h = DeviceHierarchy(max_points=4096, device=cuda)
    cases = sweeps = 0
    for mcs, L in chain_ids(which, mcs):
        for pattern, aim, c in chain_batch(which, mcs, L):
            assert c['n'] <= 4096
            want = host_tree_ex(c['lo'], c['hi'], c['w2'], c['n'], mcs, c['opt'])
            assert selects_parent(c, want[0]) == (aim > 0), (mcs, L, pattern, aim)
            assert same(want, device_tree_ex(h, cuda, c['lo'], c['hi'], c['w2'], c['n'], mcs, c['opt'])), (mcs, L, pattern, aim)
            cases += 1
        sweeps = max(sweeps, R.emul_tree_sweeps(emul, c['lo'], c['hi'], c['w2'], c['n'], mcs, c['opt'])[4])
    ns = 1 if which == 'root' else 2
    print('\nchains of %s: %d cases, lengths %s, patterns %s; %s; emulation sweeps <= %d'
          % (which, cases, R.LENGTHS, R.PATTERNS, R.describe([ns], R.switch_constants()), sweeps))
