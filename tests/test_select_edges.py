"""The 4-pass byte radix select of csrc/common.h (vg_radix_select) through its three callers -- vg_cluster_medians (staged or gathered
column), vg_cluster_median (a column of the packed ego array, three 256-thread groups) and the score percentile of
vg_cluster_filter_ex (staged or gathered scores) -- against numpy, bit for bit, at the sizes where it can go wrong: wave and group
edges (63 .. 65, 255 .. 257), the percentile's staging capacity (4096) and the medians' (12288).

One cluster per size; column j of the point rows holds value family j, so the five columns of one vg_cluster_medians launch cover
the five families.
"""
import ctypes

import numpy as np
import pytest

import filters_ref as fr

F32 = np.float32
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12287, 12288, 12289)
FAMILIES = ('gaussian', 'all_equal', 'two_values', 'neighbours', 'mixed_signs')
PERCENTILES = (0.0, 37.5, 50.0, 100.0)


def _family(rng, name, n):
    if name == 'gaussian':
        return (rng.normal(size=n) * 30 + 40).astype(F32)
    if name == 'all_equal':
        return np.full(n, -7.625, F32)
    if name == 'two_values':
        v = rng.integers(0, 2, size=n)
        v[:2] = (1, 0)[:n]                                                 # both present from n = 2 on
        return np.where(v == 1, 3.5, -1.25).astype(F32)
    if name == 'neighbours':                                               # 1.0 + k float32 steps, k < 256: one bin for three passes
        k = rng.integers(0, 256, size=n).astype(np.uint32)
        return (np.float32(1.0).view(np.uint32) + k).view(F32)
    v = np.round(rng.normal(size=n) * 8) / 4                               # multiples of 0.25 around 0: ties, both signs
    v = np.where(v >= 0, v + 0.25, v)                                      # no zero: -0.0 and 0.0 are two keys and one number
    v[:2] = (-0.75, 0.5)[:n]
    return v.astype(F32)


_CACHE = {}


def select_inputs():
    """-> X [M, 5] float32 (column j = family j; filler rows in between), index, seg: one cluster per size of SIZES."""
    if not _CACHE:
        rng = np.random.default_rng(21)
        total = sum(SIZES)
        X = rng.uniform(-50, 50, size=(total + 41, 5)).astype(F32)
        rows = rng.permutation(len(X))[:total]
        seg = np.r_[0, np.cumsum(SIZES)].astype(np.int32)
        for c, n in enumerate(SIZES):
            for j, name in enumerate(FAMILIES):
                X[rows[seg[c]:seg[c + 1]], j] = _family(rng, name, n)
        X.setflags(write=False)
        _CACHE['v'] = (X, rows.astype(np.int32), seg)
    return _CACHE['v']


def _clusters():
    X, index, seg = select_inputs()
    return [X[index[seg[c]:seg[c + 1]]] for c in range(len(SIZES))]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_select_inputs_have_the_stated_properties():
    key = lambda v: np.where(v.view(np.uint32) >> 31, ~v.view(np.uint32), v.view(np.uint32) | np.uint32(0x80000000))
    mean_path = 0
    for n, p in zip(SIZES, _clusters()):
        assert p.shape == (n, 5) and np.isfinite(p).all()
        g, eq, two, nb, mx = (p[:, j] for j in range(5))
        assert len(np.unique(eq)) == 1
        assert len(np.unique(two)) == min(n, 2)
        assert len(np.unique(key(nb) >> 8)) == 1 and nb.min() >= 1.0 and (n < 4095 or len(np.unique(nb)) == 256)
        assert not (mx == 0).any() and (n < 2 or ((mx < 0).any() and (mx > 0).any()))
        assert n < 255 or len(np.unique(mx)) < n                           # ties
        if n % 2 == 0:
            s = np.sort(p, axis=0)
            mean_path += int((s[n // 2 - 1] != s[n // 2]).sum())
    assert mean_path >= 8                                                  # even sizes whose two middle values differ
    # the sizes sit on both sides of a wave, a 256-thread group, FEX_KEY_CAP and MED_CAP (csrc/segment.hip)
    for edge in (64, 256, 4096, 12288):
        assert {edge - 1, edge, edge + 1} <= set(SIZES)


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_hip_cluster_medians_at_the_select_edges_equal_numpy(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    X, index, seg = select_inputs()
    C = len(SIZES)
    want = np.stack([np.median(p, axis=0) for p in _clusters()])
    assert want.dtype == np.float32
    d_X, d_index, d_seg = (torch.from_numpy(np.array(v)).to(cuda) for v in (X, index, seg))
    out = torch.full((C, 5), -7.0, dtype=torch.float32, device=cuda)
    check(lib.vg_cluster_medians(ptr(d_X), 5, 5, ptr(d_index), ptr(d_seg), C, ptr(out), stream_ptr()), 'vg_cluster_medians')
    got = out.cpu().numpy()
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, [(SIZES[c], FAMILIES[j], got[c, j], want[c, j]) for c, j in bad[:8]]


@pytest.mark.gpu
def test_hip_cluster_median_at_the_select_edges_equals_numpy(cuda):
    """vg_cluster_median called directly on a packed [M, 3] array: the five families as columns (0, 1, 2) and (2, 3, 4)"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    X, index, seg = select_inputs()
    C = len(SIZES)
    for cols in ((0, 1, 2), (2, 3, 4)):
        ego = np.ascontiguousarray(X[index][:, cols])
        want = np.stack([np.median(ego[seg[c]:seg[c + 1]], axis=0) for c in range(C)])
        d_ego, d_seg = torch.from_numpy(ego).to(cuda), torch.from_numpy(seg).to(cuda)
        med = torch.full((C, 3), -7.0, dtype=torch.float32, device=cuda)
        rot = torch.zeros((C, 6), dtype=torch.float64, device=cuda)
        check(lib.vg_cluster_median(ptr(d_ego), ptr(d_seg), C, ptr(med), ptr(rot), stream_ptr()), 'vg_cluster_median')
        got = med.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert len(bad) == 0, [(SIZES[c], FAMILIES[cols[j]], got[c, j], want[c, j]) for c, j in bad[:8]]


@pytest.mark.gpu
def test_hip_filter_percentile_at_the_select_edges_equals_the_restatement(cuda):
    """stats[:, 13] of vg_cluster_filter_ex with only the ephemeral filter active == filters_ref.percentile, bit for bit"""
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr, check, FilterParams, FILTER_NAMES, FILTER_AND, FILTER_NSTATS
    X, index, seg = select_inputs()
    C = len(SIZES)
    d_X, d_index, d_seg = (torch.from_numpy(np.array(v)).to(cuda) for v in (X, index, seg))
    d_plane = torch.tensor([0.0, 0.0, 1.0, 1.7], dtype=torch.float64, device=cuda)
    k = FILTER_NAMES.index('filter_by_ephemeral_score')
    for j, name in enumerate(FAMILIES):
        d_scores = torch.from_numpy(np.ascontiguousarray(X[:, j])).to(cuda)           # one score per ROW of the point array
        for pct in PERCENTILES:
            p = FilterParams()
            p.active[k], p.logic[k] = 1, FILTER_AND
            p.percentile, p.min_percentile_pp_score = pct, 0.0
            stats = torch.full((C, FILTER_NSTATS), -7.0, dtype=torch.float64, device=cuda)
            verdict = torch.zeros((C, 7), dtype=torch.uint8, device=cuda)
            valid = torch.zeros(C, dtype=torch.uint8, device=cuda)
            check(lib.vg_cluster_filter_ex(ptr(d_X), 5, ptr(d_index), ptr(d_seg), C, ptr(d_plane), ptr(d_scores), ctypes.byref(p),
                                           ptr(stats), ptr(verdict), ptr(valid), stream_ptr()), 'vg_cluster_filter_ex')
            got = stats[:, 13].cpu().numpy()
            want = np.array([fr.percentile(q[:, j], pct) for q in _clusters()], np.float64)
            bad = np.flatnonzero(_bits(got) != _bits(want))
            assert len(bad) == 0, (name, pct, [(SIZES[c], got[c], want[c]) for c in bad[:8]])
            assert np.array_equal(verdict[:, k].cpu().numpy().astype(bool), ~(want > 0.0))
