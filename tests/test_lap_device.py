"""The assignment kernel (csrc/lap.hip k_lap_groups) on the GPU: bit for bit against vg_lap_groups_host -- the same per-column text, which
tests/test_lap_host.py holds to scipy -- on every case of that file (ties, prices, prefixes, forbidden and invalid entries, empty and
wrongly described groups, both column forms, workgroups of 16 and of 4 waves), with guard words around the outputs, from a captured
graph, twice, at the size limit; and the Python forms on CUDA tensors."""
import numpy as np
import pytest

import lap_ref as R
from vilgod_amd import lap
from vilgod_amd._lib import VilgodHipError

pytestmark = pytest.mark.gpu


def _same(c, cuda, label, **kw):
    rc_h, match_h, status_h = R.host_raw(c)
    rc_d, match_d, status_d = R.device_raw(c, cuda, **kw)
    assert rc_h == 0 and rc_d == 0, label
    assert status_d.tobytes() == status_h.tobytes(), (label, status_d[:8], status_h[:8])
    assert match_d.tobytes() == match_h.tobytes(), (label, np.flatnonzero(match_d != match_h)[:5])
    assert R.guards_untouched(c, match_d, status_d), label
    return match_h, status_h


def test_every_host_case_equals_the_host_bit_for_bit(cuda):
    cases = R.all_cases()
    assert len(cases) > 50
    for name, c in cases.items():
        _same(c, cuda, name)


def test_wrongly_described_groups_are_marked_not_followed(cuda):
    """(every read an unchecked kernel would make lies inside the buffers of lap_ref._buffers)"""
    for name, c in R.bad_table_cases().items():
        _, status = _same(c, cuda, name)
        assert status[:c['n_groups']].tolist() == c['expect_status'], name


def test_call_level_refusals_launch_nothing(cuda):
    c = R.case([R.continuous(3, 3, 1)])
    for over in ({'max_rows': lap.LAP_MAX + 1}, {'max_cols': lap.LAP_MAX + 1}, {'n_groups': -1}, {'unassigned': np.nan}, {'n_snaps': 2}):
        rc, match, status = R.device_raw(dict(c, **over), cuda)
        assert rc == 1, over
        assert np.all(match == R.SENTINEL) and np.all(status == R.SENTINEL), over


@pytest.mark.parametrize('name', ['c:prefix1', 'i:prefix1', 'c:5_groups_4_waves', 'r:order_entry_repeated'])
def test_captured_graph_replays_the_same_bits(cuda, name):
    c = R.all_cases()[name]
    _same(c, cuda, name, graph=True)


@pytest.mark.parametrize('name', ['i:classic', 'i:all_equal_priced', 'c:17_groups_16_waves'])
def test_two_runs_give_the_same_bits(cuda, name):
    c = R.all_cases()[name]
    _, m1, s1 = R.device_raw(c, cuda)
    _, m2, s2 = R.device_raw(c, cuda)
    assert m1.tobytes() == m2.tobytes() and s1.tobytes() == s2.tobytes()


def test_one_problem_at_the_size_limit(cuda):
    import torch
    a = R.continuous(1024, 1024, 50)
    _same(R.case([a]), cuda, '1024 x 1024')
    _same(R.case([R.integer(1024, 1024, 51)], 1.0, orders=[R.permutation(1024, 52)], prefixes=[[1, 512, 1023, 1024]]), cuda, 'ties at 1024')
    r, cc = lap.linear_sum_assignment(torch.from_numpy(a).to(cuda))
    r2, c2 = R.scipy_lsa(a)
    assert r.is_cuda and r.dtype == torch.int64 and np.array_equal(r.cpu().numpy(), r2) and np.array_equal(cc.cpu().numpy(), c2)
    with pytest.raises(VilgodHipError, match='bad argument'):
        lap.linear_sum_assignment(torch.zeros(1025, 1025, dtype=torch.float64, device=cuda))


def test_drop_in_on_cuda_tensors(cuda):
    import torch
    for n, m in [(0, 0), (0, 3), (3, 0), (1, 1), (7, 3), (3, 7), (65, 64), (64, 257), (257, 129)]:
        for maximize in (False, True):
            a = R.continuous(n, m, 60)
            r, cc = lap.linear_sum_assignment(torch.from_numpy(a).to(cuda), maximize=maximize)
            r2, c2 = R.scipy_lsa(a, maximize=maximize)
            assert r.is_cuda and cc.is_cuda and r.dtype == cc.dtype == torch.int64
            assert np.array_equal(r.cpu().numpy(), r2) and np.array_equal(cc.cpu().numpy(), c2), (n, m)
    a = R.continuous(4, 5, 62).astype(np.float32)                            # float32 in: widened exactly
    r, cc = lap.linear_sum_assignment(torch.from_numpy(a).to(cuda))
    assert np.array_equal(cc.cpu().numpy(), R.scipy_lsa(a)[1])
    b = torch.from_numpy(R.continuous(4, 5, 62)).to(cuda)
    b[1, 2] = float('nan')
    with pytest.raises(ValueError, match='matrix contains invalid numeric entries'):
        lap.linear_sum_assignment(b)
    b[1, :] = float('inf')
    with pytest.raises(ValueError, match='cost matrix is infeasible'):
        lap.linear_sum_assignment(b)


def test_lap_groups_equals_lap_groups_host(cuda):
    import torch
    mats = [R.continuous(5, 7, 70), R.continuous(0, 3, 70), R.integer(66, 64, 70), R.continuous(3, 300, 70)]
    orders = np.concatenate([R.permutation(a.shape[0], 71) for a in mats])
    prefixes = [R.some_prefixes(a.shape[0]) for a in mats]
    flat = np.concatenate([a.reshape(-1) for a in mats])
    sizes = np.array([a.size for a in mats])
    row_off = np.cumsum([0] + [a.shape[0] for a in mats])
    col_off = np.cumsum([0] + [a.shape[1] for a in mats])
    for kw in ({}, {'unassigned_cost': 0.5}, {'unassigned_cost': 1.0, 'order': orders, 'prefixes': prefixes}):
        want = lap.lap_groups_host(flat, np.cumsum(sizes) - sizes, row_off, col_off, **kw)
        if 'order' in kw:
            kw = dict(kw, order=torch.from_numpy(orders).to(cuda))
        got = lap.lap_groups(torch.from_numpy(flat).to(cuda), np.cumsum(sizes) - sizes, row_off, col_off, **kw)
        assert got[0].is_cuda and got[3].is_cuda and got[0].dtype == torch.int32
        assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[3].cpu().numpy().tobytes() == want[3].tobytes()
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    with pytest.raises(ValueError):
        lap.lap_groups(flat, np.cumsum(sizes) - sizes, row_off, col_off)
