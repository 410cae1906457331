"""Shared by tests/test_lap_host.py, test_lap_device.py and test_eval_match.py: the cases of the linear-assignment solver as raw ABI calls
(every table an array the test owns, the matrices and the snapshots inside larger allocations, so that a call which describes a
group wrongly can be made without any read leaving the test's memory), the two runners, and the scipy references."""
import ctypes
import functools
import math

import numpy as np
from scipy.optimize import linear_sum_assignment as scipy_lsa

SIZES = (0, 1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SENTINEL = -7                       # d_match / d_status before the call
MARGIN = 2048                       # elements around the cost matrices and the snapshots (guard words; room for a misdescribed group)
INF = np.inf


def shapes():
    """squares, neighbours of the size list both ways, and a few far apart"""
    out = [(s, s) for s in SIZES]
    for a, b in zip(SIZES[:-1], SIZES[1:]):
        out += [(a, b), (b, a)]
    out += [(1, 257), (257, 1), (7, 256), (256, 7), (64, 257), (257, 64), (3, 129), (129, 3)]
    return out


def continuous(n, m, seed):
    return np.random.default_rng([seed, n, m]).uniform(0.0, 1.0, (n, m))


def integer(n, m, seed, high=4):
    return np.random.default_rng([seed, n, m, 7]).integers(0, high, (n, m)).astype(np.float64)


def permutation(n, seed):
    return np.random.default_rng([seed, n, 11]).permutation(n).astype(np.int32)


def some_prefixes(n):
    """every prefix of a small group, the edges of a large one"""
    if n <= 65:
        return list(range(1, n + 1))
    return sorted({k for k in (1, 2, 3, 63, 64, 65, 127, 128, 129, n - 1, n) if 1 <= k <= n})


# ---- raw calls -------------------------------------------------------------------------------------------------------------------
def case(mats, unassigned=INF, orders=None, prefixes=None, **over):
    """One call over the matrices `mats` (packed one behind the other with a gap of 3 elements), rows and columns numbered through.
    orders: per group a permutation or None (None for all: no order table).  prefixes: per group a list (None: one snapshot each).
    `over` replaces any field afterwards (that is how a group is described wrongly)."""
    mats = [np.asarray(a, np.float64) for a in mats]
    ns, ms = [a.shape[0] for a in mats], [a.shape[1] for a in mats]
    row_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    col_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    sizes = np.array([a.size + 3 for a in mats], np.int64)
    cost_off = (np.cumsum(sizes) - sizes).astype(np.int64)
    cost_len = int(sizes.sum())
    cost = np.full(cost_len, 0.25)
    for a, o in zip(mats, cost_off):
        cost[o:o + a.size] = a.reshape(-1)
    c = {'cost': cost, 'cost_len': cost_len, 'cost_off': cost_off, 'row_off': row_off, 'col_off': col_off, 'n_groups': len(mats),
         'max_rows': max(ns + [0]), 'max_cols': max(ms + [0]), 'unassigned': float(unassigned), 'order': None, 'n_rows': 0,
         'prefix': None, 'prefix_off': None}
    if orders is not None:
        c['order'] = np.concatenate([np.arange(n, dtype=np.int32) if o is None else np.asarray(o, np.int32) for n, o in zip(ns, orders)]
                                    + [np.zeros(0, np.int32)]).astype(np.int32)
        c['n_rows'] = len(c['order'])
    if prefixes is not None:
        counts = [len(p) for p in prefixes]
        c['prefix'] = np.concatenate([np.asarray(p, np.int32) for p in prefixes] + [np.zeros(0, np.int32)]).astype(np.int32)
        c['prefix_off'] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        per = np.repeat(np.array(ns, np.int64), counts)
    else:
        per = np.array(ns, np.int64)
    ends = np.cumsum(per + 1)                                      # one slack element behind every snapshot
    c['match_off'] = (ends - per - 1).astype(np.int64)
    c['n_snaps'] = len(per)
    c['match_len'] = int(ends[-1]) if len(ends) else 0
    c['snap_rows'] = per
    c.update(over)
    return c


def _padded(a, lo=MARGIN, hi=MARGIN, fill=0):
    buf = np.full(lo + len(a) + hi, fill, a.dtype)
    buf[lo:lo + len(a)] = a
    return buf


def _buffers(c):
    """the allocations of a call: costs and order with a margin on both sides (filled with plausible values), match with guard words"""
    cost = _padded(c['cost'], fill=0.5)
    order = None if c['order'] is None else _padded(c['order'])
    prefix = None if c['prefix'] is None else _padded(c['prefix'], fill=1)
    prefix_off = None if c['prefix_off'] is None else c['prefix_off']
    match_off = _padded(c['match_off'])
    match = np.full(c['match_len'] + 2 * MARGIN, SENTINEL, np.int32)
    status = np.full(c['n_groups'] + 8, SENTINEL, np.int32)
    return cost, order, prefix, prefix_off, match_off, match, status


def _p(a, skip=0):
    return None if a is None else ctypes.c_void_p(a.ctypes.data + skip * a.itemsize)


def host_raw(c):
    """-> (return code, match allocation [MARGIN + match_len + MARGIN], status allocation [n_groups + 8])"""
    from vilgod_amd._lib import lib
    cost, order, prefix, prefix_off, match_off, match, status = _buffers(c)
    rc = lib.vg_lap_groups_host(_p(cost, MARGIN), c['cost_len'], _p(c['cost_off']), _p(c['row_off']), _p(c['col_off']), c['n_groups'],
                                c['n_rows'], c['max_rows'], c['max_cols'], c['unassigned'], _p(order, MARGIN), _p(prefix, MARGIN),
                                _p(prefix_off), c['n_snaps'], _p(match_off, MARGIN), c['match_len'], _p(match, MARGIN), _p(status))
    return rc, match, status


def device_raw(c, cuda, graph=False):
    """the same call through vg_lap_groups; graph: captured into a torch graph and replayed twice (the outputs reset in between)"""
    import torch
    from vilgod_amd._lib import lib, stream_ptr
    host = _buffers(c)
    dev = [None if a is None else torch.from_numpy(a).to(cuda) for a in host]
    tabs = [torch.from_numpy(np.ascontiguousarray(c[k])).to(cuda) for k in ('cost_off', 'row_off', 'col_off')]
    cost, order, prefix, prefix_off, match_off, match, status = dev

    def dp(t, skip=0):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + skip * t.element_size())

    def call(stream):
        return lib.vg_lap_groups(dp(cost, MARGIN), c['cost_len'], dp(tabs[0]), dp(tabs[1]), dp(tabs[2]), c['n_groups'], c['n_rows'],
                                 c['max_rows'], c['max_cols'], c['unassigned'], dp(order, MARGIN), dp(prefix, MARGIN), dp(prefix_off),
                                 c['n_snaps'], dp(match_off, MARGIN), c['match_len'], dp(match, MARGIN), dp(status), stream_ptr(stream))
    if not graph:
        rc = call(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return rc, match.cpu().numpy(), status.cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc = call(side)                                             # warm-up outside the capture (the LDS attribute is set here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert rc == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = call(torch.cuda.current_stream())
    outs = []
    for _ in range(2):
        match.fill_(SENTINEL)
        status.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        outs.append((match.cpu().numpy(), status.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return rc, outs[0][0], outs[0][1]


def snapshots(c, match):
    """the snapshots of a call's match allocation -> [int32 array per snapshot]"""
    inner = match[MARGIN:MARGIN + c['match_len']]
    return [inner[o:o + n] for o, n in zip(c['match_off'], c['snap_rows'])]


def guards_untouched(c, match, status):
    """the guard words around d_match, the slack element behind every snapshot and the words behind d_status"""
    ok = np.all(match[:MARGIN] == SENTINEL) and np.all(match[MARGIN + c['match_len']:] == SENTINEL)
    inner = match[MARGIN:MARGIN + c['match_len']]
    ok = ok and all(inner[o + n] == SENTINEL for o, n in zip(c['match_off'], c['snap_rows']) if o >= 0 and o + n < len(inner))
    return bool(ok and np.all(status[c['n_groups']:] == SENTINEL))


# ---- references --------------------------------------------------------------------------------------------------------------------
def exact_total(a, col4row, unassigned=0.0):
    """the exact value of an assignment (col4row: -1 = unassigned at the price)"""
    col4row = np.asarray(col4row)
    terms = [a[i, j] for i, j in enumerate(col4row) if j >= 0]
    free = int(np.count_nonzero(col4row < 0))
    return math.fsum(terms + ([unassigned] * free if free else []))


def is_assignment(col4row, m):
    used = np.asarray(col4row)[np.asarray(col4row) >= 0]
    return bool(np.all(used < m) and len(np.unique(used)) == len(used))


def scipy_unassigned(a, unassigned):
    """scipy on the [n, m + n] matrix padded with the price on the dummy diagonal, +inf elsewhere -> col4row with -1 for a dummy"""
    n, m = a.shape
    if n == 0:
        return np.zeros(0, np.int64)
    pad = np.full((n, m + n), INF)
    pad[:, :m] = a
    pad[np.arange(n), m + np.arange(n)] = unassigned
    r, cc = scipy_lsa(pad)
    out = np.full(n, -1, np.int64)
    out[r] = np.where(cc < m, cc, -1)
    return out


def scipy_prefix(a, unassigned, order, k):
    """the reference for the snapshot after k rows of `order`: scipy on those rows, the others -1"""
    rows = np.asarray(order[:k], np.int64)
    out = np.full(a.shape[0], -1, np.int64)
    out[rows] = scipy_unassigned(a[rows], unassigned)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
PRICES = {'continuous': (-0.5, 0.5, 1.5), 'integer': (-1.0, 1.0, 5.0)}        # below, among and above the entries


def _forbid(a, seed, frac=0.4):
    """+inf on a share of the pairs, the diagonal kept finite (so a square or wide matrix stays feasible)"""
    a = a.copy()
    hit = np.random.default_rng([seed, 13]).uniform(size=a.shape) < frac
    hit[np.arange(min(a.shape)), np.arange(min(a.shape))] = False
    a[hit] = INF
    return a


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: call}.  'c:' continuous and 'i:' integer costs; classic (every row takes a column) calls hold the wide and square
    shapes, the priced ones every shape."""
    wide = [s for s in shapes() if s[0] <= s[1]]
    cases = {}
    cases['c:classic'] = case([continuous(n, m, 1) for n, m in wide])
    cases['i:classic'] = case([integer(n, m, 2) for n, m in wide] + [np.full((n, m), 3.0) for n, m in wide if n in (1, 7, 64, 65)])
    cases['c:tall_is_infeasible'] = case([continuous(3, 2, 3), continuous(65, 64, 3), continuous(2, 2, 3)])
    for kind, make in (('c', continuous), ('i', integer)):
        for pi, price in enumerate(PRICES['continuous' if kind == 'c' else 'integer']):
            mats = [make(n, m, 4 + pi) for n, m in shapes()]
            cases[f'{kind}:priced{pi}'] = case(mats, price)
            small = [(n, m) for n, m in shapes() if max(n, m) <= 65]
            big = [(129, 127), (257, 255), (129, 257), (256, 256)]
            mats = [make(n, m, 8 + pi) for n, m in small + big]
            cases[f'{kind}:prefix{pi}'] = case(mats, price, orders=[permutation(a.shape[0], 9) for a in mats],
                                               prefixes=[some_prefixes(a.shape[0]) for a in mats])
    cases['i:all_equal_priced'] = case([np.full((n, m), 1.0) for n, m in ((7, 7), (5, 9), (9, 5), (65, 64))], 1.0,
                                       orders=[permutation(n, 10) for n in (7, 5, 9, 65)], prefixes=[some_prefixes(n) for n in (7, 5, 9, 65)])
    # forbidden pairs
    cases['c:forbidden_feasible'] = case([_forbid(continuous(n, m, 11), n) for n, m in wide if n > 0])
    bad_row = continuous(5, 7, 12); bad_row[3, :] = INF                      # a row with no finite entry
    two_one = continuous(4, 6, 12); two_one[:2, 1:] = INF                    # two rows that can only take column 0
    cases['c:forbidden_infeasible'] = case([bad_row, continuous(3, 3, 12), two_one, _forbid(continuous(66, 70, 12), 5)])
    cases['c:forbidden_priced'] = case([bad_row, two_one, _forbid(continuous(65, 64, 12), 6)], 0.5)
    nan = continuous(4, 5, 13); nan[2, 3] = np.nan
    ninf = continuous(65, 66, 13); ninf[64, 65] = -INF
    late = continuous(3, 300, 13); late[2, 299] = np.nan                      # (the LDS form's width)
    cases['c:invalid_entries'] = case([nan, continuous(2, 2, 13), ninf, late], prefixes=[[1, 4], [2], [64, 65], [3]])
    cases['c:empty'] = case([np.zeros((0, 0)), continuous(2, 3, 14), np.zeros((0, 5)), np.zeros((4, 0)), continuous(1, 1, 14)])
    cases['c:empty_priced'] = case([np.zeros((0, 0)), np.zeros((0, 5)), np.zeros((4, 0)), continuous(1, 1, 14)], 0.0,
                                   prefixes=[[], [], [1, 2, 3, 4], [1]])
    # launch shape
    cases['c:1000_of_1x1'] = case([np.array([[float(i % 5)]]) for i in range(1000)])
    for g in (15, 16, 17, 33):
        cases[f'c:{g}_groups_16_waves'] = case([continuous(3 + i % 5, 4 + i % 7, 20 + i) for i in range(g)], 0.6)
    for g in (3, 4, 5, 9):
        cases[f'c:{g}_groups_4_waves'] = case([continuous(2 + i, 300 + i, 30 + i) if i % 2 == 0 else continuous(5 + i, 6 + i, 30 + i)
                                               for i in range(g)], 0.4 if g % 2 else INF)
    cases.update(bad_table_cases())
    return cases


def bad_table_cases():
    """every kind of wrongly described group (status -1), each in a call with sound groups around it.  Every read an unchecked kernel
    would make stays inside the allocations of _buffers: the margins hold 2048 elements on each side."""
    def base(**over):
        mats = [continuous(4, 5, 40), continuous(5, 6, 41), continuous(3, 3, 42)]
        return case(mats, 0.5, orders=[permutation(4, 1), permutation(5, 2), permutation(3, 3)], prefixes=[[2, 4], [1, 3, 5], [3]], **over)
    b = base()
    cases = {}

    def put(name, expect, **over):
        c = base(**over)
        c['expect_status'] = expect
        cases['r:' + name] = c

    def edit(key, at, value):
        a = b[key].copy()
        a[at] = value
        return {key: a}
    put('sound', [0, 0, 0])
    put('rows_above_max_rows', [0, -1, 0], max_rows=4)
    put('cols_above_max_cols', [0, -1, 0], max_cols=5)
    put('negative_rows', [0, 0, -1], **edit('row_off', 3, 8))
    put('negative_cols', [0, 0, -1], **edit('col_off', 3, 10))
    put('matrix_behind_the_costs', [0, 0, -1], cost_len=b['cost_len'] - 4)
    put('matrix_before_the_costs', [-1, 0, 0], **edit('cost_off', 0, -3))
    put('order_behind_the_table', [0, 0, -1], n_rows=b['n_rows'] - 1)
    put('order_entry_too_large', [0, -1, 0], **edit('order', 4 + 2, 5))
    put('order_entry_negative', [-1, 0, 0], **edit('order', 1, -1))
    rep = b['order'].copy(); rep[9] = rep[10]
    put('order_entry_repeated', [0, 0, -1], order=rep)
    put('prefix_zero', [-1, 0, 0], **edit('prefix', 0, 0))
    put('prefix_above_rows', [0, -1, 0], **edit('prefix', 4, 6))
    put('prefix_repeated', [0, -1, 0], **edit('prefix', 3, 1))
    put('prefix_descending', [-1, 0, 0], **edit('prefix', 1, 1))
    put('prefix_range_reversed', [0, 0, -1], **edit('prefix_off', 3, 4))       # group 2: [5, 4)
    put('prefix_range_behind_the_list', [0, 0, -1], n_snaps=5)
    put('prefix_range_negative', [-1, 0, 0], **edit('prefix_off', 0, -1))
    put('snapshot_behind_the_table', [0, 0, -1], match_len=b['match_len'] - 2)
    put('snapshot_before_the_table', [0, -1, 0], **edit('match_off', 3, -2))
    return cases
