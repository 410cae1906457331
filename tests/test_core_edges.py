"""The exact k-NN core distances (csrc/cluster_core.inc: k_cl_blocks, k_cl_core_blk, k_cl_core_far) at their work-list, tile and shell
edges.  The expected value is always core_ref.core2_dense (all pairs, float64, no tree, no cut), compared WITHOUT a tolerance: the stage is
exact by contract.  core_ref.Stage restates the stage's decisions from the geometry probe; the CPU tests use it to show that every scene
sits where its name says and that the scenes notice each synthesised fault, the GPU tests to describe a failing row and to hold the
library's own count of work items and far-phase queries (the VG_CLUSTER_DEBUG line) to the branch each case was built for."""
import os
import re
import sys
import tempfile

import numpy as np
import pytest

import core_ref as cr
import mst_ref as mr
from oracle import hdbscan_oracle as ho

Q = 2                                                                 # the row of the aimed query in the families that have one


def _inv(st):
    inv = np.empty(st.n, int)
    inv[st.order] = np.arange(st.n)
    return inv


def _restated(family, case, dim, k):
    """the account of one case; the restatement without a fault must agree with the dense reference on every row"""
    acc = cr.account(family, case, dim, k)
    want = cr.expected(family, case, dim, k)
    bad = np.flatnonzero(acc.core2 != want)
    assert bad.size == 0, (family, case, dim, k, cr.describe(acc, bad[0]), acc.core2[bad[0]], want[bad[0]])
    return acc


# ------------------------------------------------------------------------------------------------------------ CPU: the reference
@pytest.mark.parametrize('family', cr.FAMILIES)
def test_dense_reference_equals_the_oracle(family):
    """all pairs against the KD-tree cut at k + 9 neighbours: either side can then be trusted against the other"""
    for case, dim, k in cr.cases(family):
        X = cr.scene(family, case, dim, k)
        assert np.array_equal(cr.expected(family, case, dim, k), ho.core_distances_sq(X, k)), (family, case, dim, k)
    X, k = cr.small_scene()
    assert np.isinf(cr.core2_dense(X, k, 3)).all() and np.isinf(ho.core_distances_sq(X, k)).all()


def test_dense_reference_excludes_the_row_by_index_and_sums_left_to_right():
    X = np.array([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 2, 3, 4, 5], [1e-3, 3e-4, 7e-5, 0.1, 0.3]], np.float32)
    assert cr.core2_dense(X, 1, 5).tolist()[:2] == [0.0, 0.0]        # a coincident copy counts, the row itself does not
    d = X[3].astype(np.float64) - X[2].astype(np.float64)
    for dim, want in ((3, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), (4, ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]),
                      (5, (((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) + d[4] * d[4])):
        assert cr.core2_dense(X[2:], 1, dim).tolist() == [want, want]
    assert np.isinf(cr.core2_dense(X, 4, 3)).all()                   # n <= k


# ------------------------------------------------------------------------------------------------------------ CPU: the scenes are aimed
def test_scenes_are_aimed_node_m():
    for m, dim, k in cr.cases('node_m'):
        acc, st = _restated('node_m', m, dim, k), cr.stage('node_m', m, dim, k)
        rows = np.arange(2, 2 + m)
        cells = {tuple(c) for c in st.cell[_inv(st)[rows]]}
        assert len({tuple(np.array(c) >> 1) for c in cells}) == 1 and len(cells) >= 4, (m, cells)
        ent = sorted(set(acc.entry_of[rows]))
        assert all(acc.entry_of[r] not in ent for r in range(st.n) if not 2 <= r < 2 + m)        # the items hold the node alone
        if m <= cr.CLB_SPLIT:                                        # one level-1 item of ceil(m / 64) chunks
            assert [acc.entries[e][0] for e in ent] == [1] * -(-m // 64), (m, ent)
            first = acc.entries[ent[0]][1]
            assert [acc.entries[e][1] for e in ent] == [first + 64 * c for c in range(len(ent))]
        else:                                                        # 97: the cells are the items
            assert [acc.entries[e][0] for e in ent] == [0] * len(cells), (m, ent)
        assert sum(c for _, _, c in st.work_list()) == acc.n_items


def test_scenes_are_aimed_cell_m():
    for m, dim, k in cr.cases('cell_m'):
        acc, st = _restated('cell_m', m, dim, k), cr.stage('cell_m', m, dim, k)
        inv = _inv(st)
        rows = np.arange(2, 2 + m)
        assert len({tuple(c) for c in st.cell[inv[rows]]}) == 1
        s, e = st.node_range(1, st.cell[inv[2]] >> 1)
        assert e - s == m + 40 > cr.CLB_SPLIT
        ent = sorted(set(acc.entry_of[rows]))
        assert [acc.entries[x][0] for x in ent] == [0] * -(-m // 64), (m, ent)
        assert sorted(np.bincount(acc.entry_of[rows])[ent], reverse=True)[-1] == (m - 1) % 64 + 1   # the last chunk's live lanes


def test_scenes_are_aimed_shell_cap():
    for total, dim, k in cr.cases('shell_cap'):
        acc, st = _restated('shell_cap', total, dim, k), cr.stage('shell_cap', total, dim, k)
        inv = _inv(st)
        rows = np.arange(2 + total - 80, 2 + total)                  # the chosen level-1 node
        assert st.n <= 4200
        c1 = st.cell[inv[rows[0]]] >> 1
        assert st.node_range(1, c1)[1] - st.node_range(1, c1)[0] == 80
        s3, e3 = st.node_range(3, c1 >> 2)
        assert e3 - s3 == total
        ent = sorted(set(acc.entry_of[rows]))
        if total == cr.CLB_SHELL_CAP:
            assert [acc.entries[x][0] for x in ent] == [1, 1]
        else:
            assert len(ent) == len({tuple(c) for c in st.cell[inv[rows]]}) and all(acc.entries[x][0] == 0 for x in ent)
            assert all(lv == 0 for lv, s, _ in st.work_list() if s3 <= s < e3)


def test_scenes_are_aimed_tile():
    for p, dim, k in cr.cases('tile'):
        acc = _restated('tile', p, dim, k)
        ent = sorted(set(acc.entry_of[2:72]))                        # node A: 70 points, one level-1 item of two chunks (64 + 6 lanes)
        assert [acc.entries[e][0] for e in ent] == [1, 1] and [(acc.entry_of == e).sum() for e in ent] == [64, 6], (p, dim, k)
        for e in ent:
            if p == 'straddle':
                assert acc.straddle[e] and acc.pop[e] == (134 if k == 64 else 129), (dim, k, acc.pop[e])
            elif k == 64:
                assert acc.pop[e] == p and acc.straddle[e] == (p in (129, 257)), (p, dim, acc.pop[e], acc.straddle[e])
            else:
                # (256 at k = 1) the fourth node starts the second pass with every list full: the lanes next to its face still need it
                assert acc.pop[e] == p and not acc.straddle[e]
    st = cr.stage('tile', 'straddle', 3, 0)
    nbh = st.neighbourhood(1, st.cell[_inv(st)[Q]] >> 1)
    assert [e - s for _, (s, e) in nbh[:5]] == [70, 30, 29, 0, 5]    # 70 + 30 = 100: the third node covers slots 100 .. 128, one point too many


def test_scenes_are_aimed_shell_edge():
    for v, dim, k in cr.cases('shell_edge'):
        acc, st = _restated('shell_edge', v, dim, k), cr.stage('shell_edge', v, dim, k)
        X, want = cr.scene('shell_edge', v, dim, k), cr.expected('shell_edge', v, dim, k)
        inv = _inv(st)
        iN, iO = k + 2, k + 3
        r2 = st.radius2[inv[Q], 1]
        d2 = lambda i, dd=dim: cr._d2(X[Q:Q + 1, :dd].astype(np.float64), X[i:i + 1, :dd].astype(np.float64))[0, 0]
        assert acc.level[Q] == 1 and abs(np.sqrt(r2) - 1.1) < 1e-5
        assert (st.cell[inv[iO]] >> 1)[0] == (st.cell[inv[Q]] >> 1)[0] + 2                     # O: beyond the shell
        assert abs((st.cell[inv[iN]] >> 1)[0] - (st.cell[inv[Q]] >> 1)[0]) <= 1 and acc.kth_a[Q] == d2(iN)   # N: the k-th inside it
        if v == 'in':
            assert d2(iN) <= r2 and acc.done[Q] and want[Q] == d2(iN)
        elif v == 'xyz_in':
            assert d2(iN, 3) <= r2 < d2(iN) and not acc.done[Q]
        else:
            other = cr.scene('shell_edge', 'out_hi' if v == 'out_lo' else 'out_lo', dim, k)
            lo, hi = (X, other) if v == 'out_lo' else (other, X)
            assert hi[iO, 0] == mr.steps(lo[iO, 0], 1) and np.array_equal(np.delete(lo, iO, 0), np.delete(hi, iO, 0))
            assert r2 < d2(iN) and not acc.done[Q] and (acc.start[Q], acc.end[Q]) == (2, 2)
            assert (d2(iO) < d2(iN) and want[Q] == d2(iO)) if v == 'out_lo' else (d2(iO) > d2(iN) and want[Q] == d2(iN))


def test_scenes_are_aimed_far_L():
    seen = set()
    for (form, L), dim, k in cr.cases('far_L'):
        acc, st = _restated('far_L', (form, L), dim, k), cr.stage('far_L', (form, L), dim, k)
        inv = _inv(st)
        assert not acc.done[Q] and st.n == k + 3
        if form == 'inf':
            assert np.isinf(acc.kth_a[Q]) and (acc.start[Q], acc.end[Q]) == (3, L)
        elif form == 'fin':
            assert np.isfinite(acc.kth_a[Q]) and (acc.start[Q], acc.end[Q]) == (min(L, cr.LMAX), L)
        elif form == 'reset':
            inside = sum(e - s for _, (s, e) in st.neighbourhood(3, st.cell[inv[Q]] >> 3)) - 1
            assert 1 <= k // 2 <= inside < k and np.isinf(acc.kth_a[Q]) and (acc.start[Q], acc.end[Q]) == (3, 4)
        elif form == 'corner':
            assert tuple(st.cell[inv[Q]]) == (0, 0, 0) and acc.end[Q] == 4
            # the low sides are clipped: the radius is the distance to the high outer face alone
            assert np.allclose(np.sqrt(st.radius2[inv[Q], 1:]), [2 * 0.4 * (1 << l) for l in range(1, 7)], atol=0.4)
        else:
            X = cr.scene('far_L', (form, L), dim, k)
            assert X[Q, 0] > st.origin[0] + cr.NB[0] * cr.CELL + 100 and st.cell[inv[Q]][0] == cr.NB[0] - 1
            assert (st.cell[inv[3:], 0] == cr.NB[0] - 1).all() and acc.end[Q] in (3, 4)
        seen.add((form, int(acc.end[Q]), k))
    for k in cr.K10:
        assert {L for f, L, kk in seen if f == 'inf' and kk == k} == {3, 4, 5, 6, 7}
        assert {L for f, L, kk in seen if f == 'fin' and kk == k} == {2, 3, 4, 5, 6, 7}


def test_scenes_are_aimed_self():
    for (kind, e), dim, k in cr.cases('self'):
        _restated('self', (kind, e), dim, k)
        X, want = cr.scene('self', (kind, e), dim, k), cr.expected('self', (kind, e), dim, k)
        copies = np.arange(3, 3 + k + e)
        assert (X[copies, :3] == X[Q, :3]).all() and len(copies) == k + e
        if kind == 'full':
            assert (X[copies] == X[Q]).all() and (want[Q] == 0.0) == (e >= 0)
        else:
            assert (X[copies, 3] != X[Q, 3]).sum() >= len(copies) - len(copies) // 5 - 1 and want[Q] > 0.0
            assert (cr._d2(X[Q:Q + 1].astype(np.float64), np.delete(X, Q, 0).astype(np.float64)) == 0).sum() <= len(copies) // 5 + 1


# ------------------------------------------------------------------------------------------------------------ CPU: the faults are noticed
@pytest.mark.parametrize('fault', sorted(cr.FAULTS))
def test_every_synthesised_fault_changes_the_answer(fault):
    family = cr.FAULTS[fault]
    hits = []
    for case, dim, k in cr.cases(family):
        if family == 'node_m' and (dim != 3 or case not in (65, 96)):
            continue                                                 # (the other cases have no second chunk: nothing to try)
        got = cr.stage(family, case, dim, k).run(k, fault).core2
        want = cr.expected(family, case, dim, k)
        if not np.array_equal(got, want):
            hits.append((case, dim, k))
    print(fault, family, len(hits), hits[:6])
    assert hits, fault


def test_fault_names_cover_the_issue_list():
    assert len(cr.FAULTS) == 10 and set(cr.FAULTS.values()) <= set(cr.FAMILIES)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def model(cuda):
    """ONE handle for the whole file, created under VG_CLUSTER_DEBUG=1 (read at vg_cluster_create): the same kernels, plus the counts line"""
    from vilgod_amd.hdbscan import HDBSCAN
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('VG_CLUSTER_DEBUG', '1')
        m = HDBSCAN(min_cluster_size=15, min_samples=15, max_points=8192, device=cuda)
    return m


def _core2(model, cuda, X, k, dim):
    """-> (core2 [n] in input order, work items, far-phase queries): the last two from the library's own stderr line"""
    import torch
    model.min_samples = k
    Xd = torch.from_numpy(np.array(X, np.float32)).to(cuda)          # (a copy: the scenes are read-only)
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        try:
            core2 = model.mst(Xd, want_core=True, dim=dim)[3]
            torch.cuda.synchronize()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors='replace')
    m = re.search(r'core distances: n (\d+), k (\d+),.*?(\d+) \(node, 64-query\) work items, (\d+) queries left to the far phase', text)
    assert m and (int(m.group(1)), int(m.group(2))) == (len(X), k), text[-600:]
    return core2.cpu().numpy(), int(m.group(3)), int(m.group(4))


def _check(model, cuda, family, case, dim, k):
    X = cr.scene(family, case, dim, k)
    got, items, far = _core2(model, cuda, X, k, dim)
    want = cr.expected(family, case, dim, k)
    bad = np.flatnonzero(got != want)
    if bad.size:
        acc = cr.account(family, case, dim, k)
        raise AssertionError(f'{family} {case} dim {dim} k {k}: {bad.size} of {len(X)} rows differ; got {got[bad[0]]!r}, want '
                             f'{want[bad[0]]!r}; {cr.describe(acc, bad[0])}')
    if family in cr.COUNTED:
        acc = cr.account(family, case, dim, k)
        assert (items, far) == (acc.n_items, acc.n_far), (family, case, dim, k, (items, far), (acc.n_items, acc.n_far))
    return items, far


@pytest.mark.gpu
@pytest.mark.parametrize('family,dim,only', [(f, d, c) for f in cr.FAMILIES for d in sorted({d for _, d, _ in cr.cases(f)})
                                             for c in ((4096, 4097) if f == 'shell_cap' else (None,))])      # (the two large scenes: one test each)
def test_core_distances_equal_dense_reference(cuda, model, family, dim, only):
    counts = [(case, k) + _check(model, cuda, family, case, d, k) for case, d, k in cr.cases(family) if d == dim and only in (None, case)]
    assert counts
    print(family, dim, len(counts), 'cases; (case, k, items, far):', counts)


@pytest.mark.gpu
def test_one_handle_across_dimensions_and_down_to_n_le_k(cuda, model):
    """5-D, then 3-D, then 4-D on the same handle, ending on ten points at k = 15: nothing of the previous call may show"""
    for dim in (5, 3, 4):
        for family, case, k in (('node_m', 97, 33), ('tile', 257, 64), ('shell_edge', 'out_lo', 16), ('self', ('full', 0), 15),
                                ('node_m', 65, 1)):
            _check(model, cuda, family, case, dim, k)
        _check(model, cuda, 'far_L', ('fin', 6), 4, 17) if dim == 4 else _check(model, cuda, 'far_L', ('inf', 7), 3, 49)
    X, k = cr.small_scene()
    got, items, far = _core2(model, cuda, X, k, 3)
    assert np.isinf(got).all() and got.shape == (10,) and far == 10
