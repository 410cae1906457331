"""vg_lap_groups_host (csrc/lap.hip, the per-column steps of csrc/lap_step.inc run one after the other) and the Python forms on top of
it, against scipy.optimize.linear_sum_assignment: exact assignments where the optimum is unique (seeded continuous costs), exact
totals where it is not (small integers, all-equal matrices), with a price for staying unassigned, with prefix snapshots under a
permuted order, with forbidden pairs, invalid entries, empty groups and wrongly described groups.  No GPU: tests/test_lap_device.py
holds the kernel to this form bit for bit, so what is proved here is what the kernel is asked to equal."""
import numpy as np
import pytest

import lap_ref as R
from vilgod_amd import lap
from vilgod_amd._lib import VilgodHipError


@pytest.fixture(scope='module')
def solved():
    """{name: (call, snapshots, status)} of every case, through the host entry point, once"""
    out = {}
    for name, c in R.all_cases().items():
        rc, match, status = R.host_raw(c)
        assert rc == 0, name
        assert R.guards_untouched(c, match, status), name
        out[name] = (c, match, status[:c['n_groups']])
    return out


def _mats(c):
    n, m = np.diff(c['row_off']), np.diff(c['col_off'])
    return [c['cost'][o:o + a * b].reshape(a, b) for o, a, b in zip(c['cost_off'], n, m)]


def _orders(c):
    return [np.arange(a.shape[0]) if c['order'] is None else c['order'][r:r + a.shape[0]] for a, r in zip(_mats(c), c['row_off'])]


def _check_against_scipy(c, match, status, exact):
    """every snapshot of a sound call: exact -> scipy's assignment and total; otherwise a valid assignment with scipy's exact total"""
    snaps = R.snapshots(c, match)
    un = c['unassigned']
    off = np.arange(c['n_groups'] + 1) if c['prefix_off'] is None else c['prefix_off']
    checked = 0
    for g, (a, order) in enumerate(zip(_mats(c), _orders(c))):
        assert status[g] == 0, g
        for s in range(off[g], off[g + 1]):
            k = a.shape[0] if c['prefix'] is None else c['prefix'][s]
            got = snaps[s]
            want = R.scipy_prefix(a, un, order, k)
            entered = np.zeros(a.shape[0], bool)
            entered[order[:k]] = True
            assert np.all(got[~entered] == -1), (g, k)
            assert R.is_assignment(got, a.shape[1]), (g, k)
            if np.isinf(un):
                assert np.all(got[entered] >= 0), (g, k)
            rows = np.flatnonzero(entered)
            price = 0.0 if np.isinf(un) else un
            assert R.exact_total(a[rows], got[rows], price) == R.exact_total(a[rows], want[rows], price), (g, k)
            if exact:
                assert np.array_equal(got, want), (g, k, got, want)
            checked += 1
    return checked


@pytest.mark.parametrize('name', ['c:classic', 'c:priced0', 'c:priced1', 'c:priced2', 'c:prefix0', 'c:prefix1', 'c:prefix2',
                                  'c:forbidden_feasible', 'c:1000_of_1x1', 'c:15_groups_16_waves', 'c:17_groups_16_waves',
                                  'c:4_groups_4_waves', 'c:5_groups_4_waves', 'r:sound'])
def test_continuous_costs_give_scipys_assignment(solved, name):
    c, match, status = solved[name]
    assert _check_against_scipy(c, match, status, exact=name != 'c:1000_of_1x1') >= 3


@pytest.mark.parametrize('name', ['i:classic', 'i:priced0', 'i:priced1', 'i:priced2', 'i:prefix0', 'i:prefix1', 'i:prefix2',
                                  'i:all_equal_priced'])
def test_integer_costs_give_scipys_total(solved, name):
    c, match, status = solved[name]
    assert _check_against_scipy(c, match, status, exact=False) >= 3


def test_the_tie_rule_free_column_first_then_lowest_index():
    """all-equal costs: row k takes the lowest free column; with the price equal to the cost the real column (in front of "stay
    unassigned") wins"""
    for un in (R.INF, 1.0):
        c = R.case([np.full((4, 6), 1.0)], un)
        _, match, status = R.host_raw(c)
        assert status[0] == 0 and R.snapshots(c, match)[0].tolist() == [0, 1, 2, 3]
    c = R.case([np.full((4, 2), 1.0)], 1.0)
    _, match, _ = R.host_raw(c)
    assert R.snapshots(c, match)[0].tolist() == [0, 1, -1, -1]


def test_statuses_and_their_fill(solved):
    c, match, status = solved['c:tall_is_infeasible']
    assert status.tolist() == [1, 1, 0]
    c, match, status = solved['c:forbidden_infeasible']
    assert status.tolist() == [1, 0, 1, 0]
    snaps = R.snapshots(c, match)
    assert np.all(snaps[0] == -1) and np.all(snaps[2] == -1) and np.all(snaps[1] >= 0)
    c, match, status = solved['c:forbidden_priced']                          # with a price nothing is infeasible
    assert status.tolist() == [0, 0, 0]
    snaps = R.snapshots(c, match)
    assert snaps[0][3] == -1 and np.count_nonzero(snaps[1][:2] >= 0) <= 1
    assert _check_against_scipy(c, match, status, exact=True) == 3
    c, match, status = solved['c:invalid_entries']
    assert status.tolist() == [2, 0, 2, 2]
    snaps = R.snapshots(c, match)
    assert all(np.all(snaps[s] == -1) for s in (0, 1, 3, 4, 5)) and np.all(snaps[2] >= 0)
    c, match, status = solved['c:empty']                                     # (4, 0) without a price: no column to take
    assert status.tolist() == [0, 0, 0, 1, 0]
    c, match, status = solved['c:empty_priced']
    assert status.tolist() == [0, 0, 0, 0]
    snaps = R.snapshots(c, match)
    assert len(snaps) == 5 and all(np.all(s == -1) for s in snaps[:4]) and snaps[4].tolist() == [-1]      # (the price 0 is below the one cost)


def test_wrongly_described_groups(solved):
    names = [n for n in solved if n.startswith('r:')]
    assert len(names) >= 20
    sound = R.snapshots(*solved['r:sound'][:2])
    for name in names:
        c, match, status = solved[name]
        assert status.tolist() == c['expect_status'], name
        if name in ('r:snapshot_before_the_table', 'r:snapshot_behind_the_table', 'r:prefix_range_behind_the_list',
                    'r:prefix_range_negative', 'r:prefix_range_reversed'):
            continue                                                       # (the snapshots themselves are displaced)
        off = c['prefix_off']
        snaps = R.snapshots(c, match)
        for g, st in enumerate(status):
            for s in range(off[g], off[g + 1]):
                if st == 0:
                    assert np.array_equal(snaps[s], sound[s]), (name, s)     # a sound group is solved whatever stands next to it
                else:
                    fill = min(max(int(c['row_off'][g + 1]) - int(c['row_off'][g]), 0), c['max_rows'], len(snaps[s]))
                    assert np.all(snaps[s][:fill] == -1), (name, s)


def test_call_level_refusals():
    c = R.case([R.continuous(3, 3, 1)])
    for over in ({'max_rows': lap.LAP_MAX + 1}, {'max_cols': lap.LAP_MAX + 1}, {'max_rows': -1}, {'n_groups': -1}, {'cost_len': -1},
                 {'match_len': -1}, {'unassigned': np.nan}, {'unassigned': -np.inf}, {'n_snaps': 2}, {'prefix': np.ones(1, np.int32)}):
        rc, match, status = R.host_raw(dict(c, **over))
        assert rc == 1, over
        assert np.all(match == R.SENTINEL) and np.all(status == R.SENTINEL), over
    rc, match, status = R.host_raw(dict(c, n_groups=0, n_snaps=0))
    assert rc == 0 and np.all(match == R.SENTINEL)


def test_one_problem_at_the_size_limit_and_one_above():
    assert lap.LAP_MAX == 1024
    a = R.continuous(1024, 1024, 50)
    r, cc = lap.linear_sum_assignment(a)
    r2, c2 = R.scipy_lsa(a)
    assert np.array_equal(r, r2) and np.array_equal(cc, c2)
    with pytest.raises(VilgodHipError, match='bad argument'):
        lap.linear_sum_assignment(R.continuous(1025, 1025, 50))
    with pytest.raises(VilgodHipError, match='bad argument'):
        lap.linear_sum_assignment(R.continuous(3, 1025, 50))


# ---- the Python forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maximize', [False, True])
def test_drop_in_equals_scipy_on_every_shape(maximize):
    for n, m in R.shapes():
        a = R.continuous(n, m, 60)
        r, cc = lap.linear_sum_assignment(a, maximize=maximize)
        r2, c2 = R.scipy_lsa(a, maximize=maximize)
        assert r.dtype == np.int64 and cc.dtype == np.int64 and r.shape == r2.shape == cc.shape
        assert np.array_equal(r, r2) and np.array_equal(cc, c2), (n, m)
        b = R.integer(n, m, 61)
        r, cc = lap.linear_sum_assignment(b, maximize=maximize)
        r2, c2 = R.scipy_lsa(b, maximize=maximize)
        assert len(r) == min(n, m) and np.all(np.diff(r) > 0) and len(np.unique(cc)) == len(cc), (n, m)
        assert b[r, cc].sum() == b[r2, c2].sum(), (n, m)                   # (small integers: the float sum is exact)


def test_drop_in_errors_are_scipys():
    a = R.continuous(4, 5, 62)
    for bad in (np.nan, -np.inf):
        b = a.copy()
        b[1, 2] = bad
        with pytest.raises(ValueError, match='matrix contains invalid numeric entries'):
            lap.linear_sum_assignment(b)
        with pytest.raises(ValueError, match='matrix contains invalid numeric entries'):
            R.scipy_lsa(b)
    b = a.copy()
    b[2, :] = np.inf
    with pytest.raises(ValueError, match='cost matrix is infeasible'):
        lap.linear_sum_assignment(b)
    with pytest.raises(ValueError, match='cost matrix is infeasible'):
        R.scipy_lsa(b)
    with pytest.raises(ValueError, match='cost matrix is infeasible'):
        lap.linear_sum_assignment(b.T)                                      # (a forbidden column of the tall form)
    with pytest.raises(ValueError):
        lap.linear_sum_assignment(np.zeros(3))
    r, cc = lap.linear_sum_assignment(np.array([[4, 1, 3], [2, 0, 5], [3, 2, 2]]))      # scipy's own example, integers in
    assert r.tolist() == [0, 1, 2] and cc.tolist() == [1, 0, 2]


def test_lap_groups_host_lays_out_what_the_raw_call_gives():
    mats = [R.continuous(5, 7, 70), R.continuous(0, 3, 70), R.continuous(66, 64, 70)]
    orders = [R.permutation(a.shape[0], 71) for a in mats]
    prefixes = [R.some_prefixes(a.shape[0]) for a in mats]
    flat = np.concatenate([a.reshape(-1) for a in mats])
    sizes = np.array([a.size for a in mats])
    row_off = np.cumsum([0] + [a.shape[0] for a in mats])
    col_off = np.cumsum([0] + [a.shape[1] for a in mats])
    match, match_off, snap_off, status = lap.lap_groups_host(flat, np.cumsum(sizes) - sizes, row_off, col_off, 0.5, np.concatenate(orders),
                                                             prefixes)
    assert status.tolist() == [0, 0, 0] and snap_off.tolist() == [0, 5, 5, 5 + len(prefixes[2])]
    c = R.case(mats, 0.5, orders, prefixes)
    _, raw, _ = R.host_raw(c)
    for s, want in enumerate(R.snapshots(c, raw)):
        assert np.array_equal(match[match_off[s]:match_off[s] + len(want)], want), s
    match, match_off, snap_off, status = lap.lap_groups_host(flat, np.cumsum(sizes) - sizes, row_off, col_off, 0.5)
    assert snap_off.tolist() == [0, 1, 2, 3] and len(match) == 71 and status.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        lap.lap_groups_host(flat, [0], row_off, col_off)
