"""HDBSCAN's cluster-selection options -- cluster_selection_method='leaf', allow_single_cluster, max_cluster_size -- in the three forms of the
hierarchy stage: csrc/hdbscan_tree.cpp (host), csrc/hdbscan_device.hip / .inc (device) and the CPU emulation of the device form.

CPU: the host stage (vg_hdbscan_tree_host_ex) against scikit-learn's own tree code on the same minimum spanning tree
(tests/hdbscan_select_ref.py: same partition, same noise set, probabilities within 1e-9 -- measured: 0.0 on every case); the emulation
of the device rules (tests/emul/hdbscan_select_emul.cpp) against the host stage bit for bit.
GPU: the kernels (vg_hdbscan_tree_device_ex) against the host stage bit for bit, `HDBSCAN.fit` in both hierarchy modes, and one frame
through the pipeline with leaf selection in both pack modes.  The GPU tests read neither scikit-learn nor the reference tree: the host
stage, pinned on the CPU, is their yardstick."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SRC = os.path.join(ROOT, 'tests', 'emul', 'hdbscan_select_emul.cpp')
EMUL_DIR = os.path.join(ROOT, 'tests', 'emul', '_build')
MCS = 15

# (cluster_selection_method, allow_single_cluster, cluster_selection_epsilon, max_cluster_size)
EOM, LEAF, EOM_MAX200, EOM_SINGLE = ('eom', False, 0.0, 0), ('leaf', False, 0.0, 0), ('eom', False, 0.0, 200), ('eom', True, 0.0, 0)
LEAF_EPS06, LEAF_EPS5, LEAF_EPS5_SINGLE = ('leaf', False, 0.6, 0), ('leaf', False, 5.0, 0), ('leaf', True, 5.0, 0)
EOM_SINGLE_EPS08, LEAF_SINGLE = ('eom', True, 0.8, 0), ('leaf', True, 0.0, 0)
OPTION_SETS = [EOM, LEAF, EOM_MAX200, EOM_SINGLE, LEAF_EPS06, LEAF_EPS5, LEAF_EPS5_SINGLE, EOM_SINGLE_EPS08, LEAF_SINGLE]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _sel(opt):
    method, single, eps, max_size = opt
    return 1 if method == 'leaf' else 0, int(single), int(max_size)


def host_tree_ex(lo, hi, w2, n, mcs, opt):
    from vilgod_amd._lib import lib, check
    labels = np.empty(n, np.int32)
    probs = np.empty(n, np.float64)
    nc = ctypes.c_int32(0)
    check(lib.vg_hdbscan_tree_host_ex(_p(lo), _p(hi), _p(w2), n, mcs, ctypes.c_double(opt[2]), *_sel(opt), _p(labels), _p(probs), ctypes.byref(nc)),
          'vg_hdbscan_tree_host_ex')
    return labels, probs, nc.value


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def scene(seed):
    """three groups of three blobs (the blobs of a group 1.6 apart, the groups 12 apart) in uniform clutter: excess of mass selects the
    groups, leaf the blobs"""
    rng = np.random.default_rng(seed)
    pts = [rng.normal(size=(120, 3)) * 0.25 + np.add(g, o)
           for g in ((0, 0, 0), (12, 0, 0), (0, 12, 0)) for o in ((0, 0, 0), (1.6, 0, 0), (0, 1.6, 0))]
    pts.append(rng.uniform(-4, 16, size=(300, 3)))
    X = np.concatenate(pts).astype(np.float32)
    assert len(np.unique(X, axis=0)) == len(X)                      # no duplicate points
    return X


def blob(seed=0):
    return np.random.default_rng(seed).normal(size=(400, 3)).astype(np.float32)


_MST = {}


def scene_mst(name, seed):
    import hdbscan_select_ref as ref
    if (name, seed) not in _MST:
        X = scene(seed) if name == 'scene' else blob(seed)
        _MST[(name, seed)] = ref.sorted_mst(X, MCS) + (len(X),)
    return _MST[(name, seed)]


def _counts(labels):
    return len(set(labels[labels >= 0].tolist())), int((labels < 0).sum())


# ---- CPU: the reference separates the options; the host stage equals it ------------------------------------------------------------------
def test_reference_separates_the_options_on_the_scene():
    import hdbscan_select_ref as ref
    lo, hi, w2, n = scene_mst('scene', 3)
    got = {opt: _counts(ref.tree_to_labels(lo, hi, w2, MCS, opt[0], opt[1], opt[2], opt[3])[0]) for opt in OPTION_SETS[:7]}
    print(got)
    assert got[EOM] == (3, 248)
    assert got[LEAF] == (9, 361)
    assert got[EOM_MAX200] == (9, 361)
    assert got[EOM_SINGLE][0] == 3
    assert got[LEAF_EPS06][0] == 3
    assert got[LEAF_EPS5] == (2, 163)
    assert got[LEAF_EPS5_SINGLE] == (1, 125)


def test_reference_on_a_single_blob():
    import hdbscan_select_ref as ref
    lo, hi, w2, n = scene_mst('blob', 0)
    clusters = lambda opt: _counts(ref.tree_to_labels(lo, hi, w2, MCS, *opt)[0])[0]
    assert clusters(EOM) == 0
    assert clusters(EOM_SINGLE) == 1
    assert clusters(EOM_SINGLE_EPS08) == 1
    assert clusters(LEAF) == 0 and clusters(LEAF_SINGLE) == 0


@pytest.mark.parametrize('name,seed', [('scene', 3), ('blob', 0)] + [('scene', s) for s in (4, 5, 6, 7, 8)])
def test_host_stage_equals_scikit_learn(name, seed):
    import hdbscan_select_ref as ref
    from oracle import hdbscan_oracle as ho
    lo, hi, w2, n = scene_mst(name, seed)
    for opt in OPTION_SETS:
        want_l, want_p = ref.tree_to_labels(lo, hi, w2, MCS, *opt)
        got_l, got_p, nc = host_tree_ex(lo, hi, w2, n, MCS, opt)
        diff = float(np.abs(got_p - want_p).max())
        print(name, seed, opt, _counts(want_l), 'probability difference', diff)
        assert np.array_equal(got_l < 0, want_l < 0), opt                                     # the noise set
        assert np.array_equal(ho.canonical(got_l), ho.canonical(want_l)), opt                 # the partition
        assert diff <= 1e-9, opt
        if nc != len(set(want_l[want_l >= 0].tolist())):                                      # a selected root may hold no point at all
            assert opt[1] and nc == 1 and (want_l < 0).all(), opt


def test_default_options_are_the_plain_entry_point():
    from vilgod_amd._lib import lib, check
    for name, seed in (('scene', 3), ('blob', 0)):
        lo, hi, w2, n = scene_mst(name, seed)
        for eps in (0.0, 0.15):
            labels, probs, nc = np.empty(n, np.int32), np.empty(n, np.float64), ctypes.c_int32(0)
            check(lib.vg_hdbscan_tree_host(_p(lo), _p(hi), _p(w2), n, MCS, ctypes.c_double(eps), _p(labels), _p(probs), ctypes.byref(nc)))
            L, P, c = host_tree_ex(lo, hi, w2, n, MCS, ('eom', False, eps, 0))
            assert c == nc.value and np.array_equal(L, labels) and np.array_equal(P.view(np.uint64), probs.view(np.uint64))


def test_entry_points_refuse_arguments_out_of_range():
    from vilgod_amd._lib import lib
    lo, hi, w2, n = scene_mst('blob', 0)
    labels, probs, nc = np.empty(n, np.int32), np.empty(n, np.float64), ctypes.c_int32(0)
    for sel in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, -1)):
        assert lib.vg_hdbscan_tree_host_ex(_p(lo), _p(hi), _p(w2), n, MCS, ctypes.c_double(0.0), *sel, _p(labels), _p(probs), ctypes.byref(nc)) == 1, sel


def test_constructor_options():
    """what the constructor does with the three options before it touches the GPU (tests/test_hdbscan_selection.py's GPU part builds models)"""
    from vilgod_amd.hdbscan import HDBSCAN, selection_options
    assert selection_options() == (0, 0, 0)                                                   # the defaults: vg_hdbscan_tree_host
    assert selection_options('leaf', True, 200) == (1, 1, 200)
    assert selection_options('eom', False, None) == (0, 0, 0) and selection_options('eom', 0, 0) == (0, 0, 0)
    for bad in (dict(cluster_selection_method='mean'), dict(cluster_selection_method=None), dict(max_cluster_size=-1)):
        with pytest.raises(ValueError):
            selection_options(**bad)
        with pytest.raises(ValueError):
            HDBSCAN(min_cluster_size=15, device='cpu', **bad)                                 # (refused before any handle is made)


# ---- CPU: the rules of the device formulation against the host stage, bit for bit ---------------------------------------------------------
@pytest.fixture(scope='module')
def emul():
    os.makedirs(EMUL_DIR, exist_ok=True)
    so = os.path.join(EMUL_DIR, 'libhd_select_emul.so')
    inc = os.path.join(ROOT, 'vilgod_amd', 'csrc', 'hdbscan_device.inc')
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(EMUL_SRC), os.path.getmtime(inc)):
        subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-I', os.path.dirname(inc), EMUL_SRC, '-o', so], check=True)
    lib = ctypes.CDLL(so)
    lib.hd_emul_tree_ex.restype = ctypes.c_int
    return lib


def emul_tree_ex(lib, lo, hi, w2, n, mcs, opt):
    labels = np.empty(n, np.int32)
    probs = np.empty(n, np.float64)
    nc, ns, sw = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.hd_emul_tree_ex(_p(lo), _p(hi), _p(w2), n, mcs, ctypes.c_double(opt[2]), *_sel(opt), _p(labels), _p(probs), ctypes.byref(nc),
                             ctypes.byref(ns), ctypes.byref(sw))
    assert rc == 0, rc
    return labels, probs, nc.value, ns.value


def random_tree(rng, n, kind):
    """-> (lo, hi, w2) sorted by w2 ONLY (ties in arbitrary order, as the GPU's edge sort leaves them).  The generators of
    tests/test_hierarchy.py: random attachment, blobs, a path, stars, a caterpillar; kind 5: every weight zero."""
    if kind in (0, 5):                           # random attachment
        lo = np.array([rng.integers(0, i) for i in range(1, n)], np.int64)
        hi = np.arange(1, n)
        w = rng.random(n - 1)
    elif kind == 1:                              # blobs: the mutual-reachability tree of a 2-D point set
        from scipy.sparse.csgraph import minimum_spanning_tree
        from scipy.spatial.distance import cdist
        c = rng.normal(size=(max(2, n // 60), 2)) * 8
        P = c[rng.integers(0, len(c), n)] + rng.normal(size=(n, 2))
        D = cdist(P, P)
        core = np.sort(D, axis=1)[:, min(5, n - 1)]
        R = np.maximum(D, np.maximum(core[:, None], core[None, :]))
        np.fill_diagonal(R, 0)
        T = minimum_spanning_tree(R).tocoo()
        lo, hi, w = T.row.astype(np.int64), T.col.astype(np.int64), T.data
    elif kind == 2:                              # a path
        lo, hi = np.arange(n - 1), np.arange(1, n)
        w = rng.random(n - 1)
    elif kind == 3:                              # a few hubs (stars joined in a chain): long adjacency lists
        hubs = max(1, n // 200)
        lo = np.array([i - 1 if i <= hubs else rng.integers(0, hubs) for i in range(1, n)], np.int64)
        lo[0] = 0
        hi = np.arange(1, n)
        w = rng.random(n - 1)
    else:                                        # a caterpillar of blobs with growing gaps: a deep split tree
        lo = np.array([rng.integers(max(0, i - 3), i) for i in range(1, n)], np.int64)
        hi = np.arange(1, n)
        w = rng.random(n - 1) * 0.1
        step = max(8, n // 40)
        w[step::step] = 1.0 + np.arange(len(w[step::step])) * 0.01
    perm = rng.permutation(n)
    lo, hi = perm[lo], perm[hi]
    l2, h2 = np.minimum(lo, hi).astype(np.int32), np.maximum(lo, hi).astype(np.int32)
    if kind != 1 and rng.random() < 0.5:
        w = np.round(w * 20) / 20               # many ties, zeros included
    if kind == 5:
        w = np.zeros(n - 1)                     # all points coincide: every lambda infinite, the root's stability too
    w2 = (w * w).astype(np.float64)
    # shuffle inside runs of equal weight: the device entry must not depend on the order of ties
    sh = rng.permutation(len(w2))
    order = sh[np.argsort(w2[sh], kind='stable')]
    return np.ascontiguousarray(l2[order]), np.ascontiguousarray(h2[order]), np.ascontiguousarray(w2[order])


TREES = [(0, 300), (1, 400), (2, 500), (3, 700), (4, 900), (0, 2500), (1, 1200), (2, 64), (3, 3000), (4, 4000), (0, 17), (2, 33), (5, 200), (5, 40),
         (0, 8), (2, 15), (0, 2)]


def tree_cases():
    """every option set (its own epsilon aside) x min_cluster_size {2, 5, 15, 32} x epsilon {0, 0.15}"""
    for method, single, _, max_size in OPTION_SETS:
        for mcs in (2, 5, 15, 32):
            for eps in (0.0, 0.15):
                yield mcs, (method, single, eps, max_size)


@pytest.mark.parametrize('seed,kind,n', [(s, k, n) for s, (k, n) in enumerate(TREES)])
def test_rules_of_the_device_formulation_equal_the_host_stage(emul, seed, kind, n):
    rng = np.random.default_rng(2000 + seed)
    lo, hi, w2 = random_tree(rng, n, kind)
    seen = set()
    for mcs, opt in tree_cases():
        for o in (opt, opt[:3] + (max(mcs, n // 10),)) if opt[3] else (opt,):                  # (a size limit that bites on this tree too)
            L0, P0, c0 = host_tree_ex(lo, hi, w2, n, mcs, o)
            L1, P1, c1, ns = emul_tree_ex(emul, lo, hi, w2, n, mcs, o)
            assert c0 == c1, (mcs, o)
            assert np.array_equal(L0, L1), (mcs, o)
            assert np.array_equal(P0.view(np.uint64), P1.view(np.uint64)), (mcs, o)            # bit for bit
            assert ns <= n // mcs
            assert c0 <= n // mcs + 1                                                          # the device packer's label bound
            seen.add((o[0], o[1], c0 > 0))
    if n >= 200 and kind != 5:
        assert ('eom', True, True) in seen                                                     # (the options did select something)


def test_no_split_trees_with_allow_single_cluster(emul):
    """a tree without a split: the root alone, by excess of mass with allow_single_cluster; nothing under leaf.  Below min_cluster_size
    points the tree has no chain node either: every point is a row of the root."""
    rng = np.random.default_rng(7)
    for n, mcs in [(2, 2), (3, 5), (15, 15), (16, 15), (29, 15), (40, 32)]:
        lo, hi, w2 = random_tree(rng, n, 2)
        for eps in (0.0, 0.15, 2.0):
            L0, P0, c0 = host_tree_ex(lo, hi, w2, n, mcs, ('eom', True, eps, 0))
            L1, P1, c1, ns = emul_tree_ex(emul, lo, hi, w2, n, mcs, ('eom', True, eps, 0))
            assert ns == 0 and c0 == c1 == 1 and np.array_equal(L0, L1) and np.array_equal(P0.view(np.uint64), P1.view(np.uint64)), (n, mcs, eps)
            assert set(L0.tolist()) <= {0, -1}
            if eps == 0.0:
                assert (L0 == 0).any()
            if eps == 2.0:
                assert (L0 == 0).all()                                                         # every lambda is above 1 / 2 (weights < 1)
            for opt in (('leaf', True, eps, 0), ('eom', False, eps, 0)):
                L, P, c = host_tree_ex(lo, hi, w2, n, mcs, opt)
                Le, Pe, ce, _ = emul_tree_ex(emul, lo, hi, w2, n, mcs, opt)
                assert c == ce == 0 and (L == -1).all() and (Le == -1).all() and (P == 0).all() and (Pe == 0).all(), (n, mcs, opt)


def test_the_existing_emulation_still_builds_on_the_extended_rules():
    """tests/emul/hdbscan_device_emul.cpp fills its view with `HdView v{}`: the new fields' zero value is the behaviour it checks"""
    src = open(os.path.join(ROOT, 'vilgod_amd', 'csrc', 'hdbscan_device.inc')).read()
    for name in ('int leaf;', 'int allow_single;', 'int max_size;', 'hd_select_eom(const HdView& v, int c)', 'hd_eps_candidates(const HdView& v, int c)',
                 'hd_eps_select(const HdView& v, int c)', 'hd_selected_by_final(const HdView& v, int c, bool use_eps)', 'hd_owner(const HdView& v, int c)',
                 'hd_point(const HdView& v, int p)', 'hd_up_all(const HdView& v, int k, int sweep)', 'hd_chain_stats(const HdView& v, int c)'):
        assert name in src, name


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def device_tree_ex(h, dev, lo, hi, w2, n, mcs, opt):
    import torch
    labels, probs, nc = h.tree(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), torch.from_numpy(w2).to(dev), n, mcs, opt[2], None, *_sel(opt))
    return labels.cpu().numpy(), probs.cpu().numpy(), nc


@pytest.mark.gpu
@pytest.mark.parametrize('seed,kind,n', [(s, k, n) for s, (k, n) in enumerate(TREES)] + [(90, 1, 2000), (91, 4, 60000), (92, 0, 150000)])
def test_device_stage_equals_host_stage(cuda, seed, kind, n):
    from vilgod_amd.hdbscan import DeviceHierarchy
    rng = np.random.default_rng(2000 + seed)
    lo, hi, w2 = random_tree(rng, n, kind)
    h = DeviceHierarchy(max_points=max(n, 64), device=cuda)
    for mcs, opt in tree_cases():
        if n > 10000 and (mcs not in (5, 15) or opt[2] != 0.15):                               # (the large trees: two sizes, one epsilon)
            continue
        for o in (opt, opt[:3] + (max(mcs, n // 10),)) if opt[3] else (opt,):
            L0, P0, c0 = host_tree_ex(lo, hi, w2, n, mcs, o)
            L1, P1, c1 = device_tree_ex(h, cuda, lo, hi, w2, n, mcs, o)
            assert c0 == c1, (mcs, o)
            assert np.array_equal(L0, L1), (mcs, o)
            assert np.array_equal(P0.view(np.uint64), P1.view(np.uint64)), (mcs, o)


@pytest.mark.gpu
def test_device_stage_on_no_split_trees_and_bad_arguments(cuda):
    from vilgod_amd.hdbscan import DeviceHierarchy
    h = DeviceHierarchy(max_points=64, device=cuda)
    rng = np.random.default_rng(7)
    for n, mcs in [(2, 2), (3, 5), (15, 15), (16, 15), (29, 15), (40, 32)]:
        lo, hi, w2 = random_tree(rng, n, 2)
        for eps in (0.0, 0.15, 2.0):
            for opt in (('eom', True, eps, 0), ('leaf', True, eps, 0), ('eom', False, eps, 0), ('eom', True, eps, 3)):
                L0, P0, c0 = host_tree_ex(lo, hi, w2, n, mcs, opt)
                L1, P1, c1 = device_tree_ex(h, cuda, lo, hi, w2, n, mcs, opt)
                assert c0 == c1 and np.array_equal(L0, L1) and np.array_equal(P0.view(np.uint64), P1.view(np.uint64)), (n, mcs, opt)
                assert c0 == (1 if opt[0] == 'eom' and opt[1] else 0)
    lo, hi, w2 = random_tree(rng, 40, 0)
    for sel in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, 0, -1)):
        with pytest.raises(RuntimeError):
            h.tree(*_dev(cuda, lo, hi, w2), 40, 5, 0.0, None, *sel)


def _dev(dev, *arrays):
    import torch
    return [torch.from_numpy(a).to(dev) for a in arrays]


@pytest.mark.gpu
def test_fit_in_both_hierarchy_modes_equals_the_host_stage(cuda):
    import torch
    from vilgod_amd.hdbscan import HDBSCAN
    X = scene(3)
    n = len(X)
    plain = {}
    for hierarchy in ('host', 'device'):
        m = HDBSCAN(min_cluster_size=MCS, cluster_selection_epsilon=0.15, max_points=2048, device=cuda, hierarchy=hierarchy).fit(X)
        plain[hierarchy] = (m.labels_.copy(), m.probabilities_.copy())
    assert np.array_equal(plain['host'][0], plain['device'][0]) and np.array_equal(plain['host'][1], plain['device'][1])
    d = HDBSCAN(min_cluster_size=MCS, cluster_selection_epsilon=0.15, max_points=2048, device=cuda, hierarchy='device', cluster_selection_method='eom',
                allow_single_cluster=False, max_cluster_size=None).fit(X)
    assert np.array_equal(d.labels_, plain['device'][0]) and np.array_equal(d.probabilities_.view(np.uint64), plain['device'][1].view(np.uint64))
    counts = {}
    for opt in OPTION_SETS:
        for hierarchy in ('host', 'device'):
            m = HDBSCAN(min_cluster_size=MCS, cluster_selection_epsilon=opt[2], max_points=2048, device=cuda, hierarchy=hierarchy,
                        cluster_selection_method=opt[0], allow_single_cluster=opt[1], max_cluster_size=opt[3] or None)
            assert m.hierarchy == hierarchy and m.selection_args == _sel(opt)
            m.fit(X)
            lo, hi, w2 = m.mst(torch.from_numpy(X).to(cuda))
            L, P, c = host_tree_ex(lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy(), n, MCS, opt)
            assert m.labels_.dtype == np.int64 and np.array_equal(m.labels_, L), (opt, hierarchy)
            assert np.array_equal(m.probabilities_.view(np.uint64), P.view(np.uint64)), (opt, hierarchy)
            counts[opt] = _counts(L)
    # the counts the scikit-learn reference gives on this scene (pinned on the CPU above, on the oracle's tree of the same points)
    assert counts[EOM] == (3, 248) and counts[LEAF] == (9, 361) and counts[EOM_MAX200] == (9, 361) and counts[LEAF_EPS5_SINGLE] == (1, 125)
    b = HDBSCAN(min_cluster_size=MCS, max_points=2048, device=cuda, hierarchy='device', allow_single_cluster=True).fit(blob(0))
    assert set(b.labels_.tolist()) == {0, -1}
    assert (HDBSCAN(min_cluster_size=MCS, max_points=2048, device=cuda, hierarchy='device').fit(blob(0)).labels_ == -1).all()


@pytest.mark.gpu
def test_pipeline_with_leaf_selection_equal_in_both_pack_modes(cuda):
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['clustering']['model'] = dict(cfg['clustering']['model'], cluster_selection_method='leaf')
    base = PseudoLabelPipeline(default_preprocessor_cfg(), device=cuda, clip_model_path='/nonexistent', vit_dtype='f16', max_points=25_000)
    host = PseudoLabelPipeline(cfg, device=cuda, clip_model_path='/nonexistent', clip=base.clip, vit_dtype='f16', max_points=25_000)
    dev = PseudoLabelPipeline(cfg, device=cuda, clip_model_path='/nonexistent', clip=base.clip, pack='device', vit_dtype='f16', max_points=25_000)
    hh = PseudoLabelPipeline(cfg, device=cuda, clip_model_path='/nonexistent', clip=base.clip, hierarchy='host', vit_dtype='f16', max_points=25_000)
    assert host.pack == 'host' and dev.pack == 'device' and host.hierarchy == dev.hierarchy and hh.hierarchy == 'host'
    assert host.cluster_model.cluster_selection_method == dev.cluster_model.cluster_selection_method == 'leaf'
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    f0, _ = base.process_frame(pts, poses[1], poses[0], fnr=1)
    fa, ra = host.process_frame(pts, poses[1], poses[0], fnr=1)
    pa = host.last_probs
    fb, rb = dev.process_frame(pts, poses[1], poses[0], fnr=1)
    pb = dev.last_probs
    fh, _ = hh.process_frame(pts, poses[1], poses[0], fnr=1)
    for k in ('cluster_ids', 'index', 'seg_off', 'valid'):
        assert np.array_equal(getattr(fa, k), getattr(fh, k)), k   # the host hierarchy stage: the same clusters
    assert fa.n_detections > 5 and fa.valid.sum() > 2
    assert fa.n_detections >= f0.n_detections                       # the leaves: at least as many clusters as the excess of mass selects
    for k in ('cluster_ids', 'index', 'seg_off', 'valid', 'static', 'tid', 'static_track'):
        x, y = getattr(fa, k), getattr(fb, k)
        assert x.dtype == y.dtype and np.array_equal(x, y), k
    assert np.array_equal(fa.ground_point_indices, fb.ground_point_indices)
    assert fa.filtered == fb.filtered and set(fa.filter_dict) == set(fb.filter_dict)
    for k in fa.filter_dict:
        assert np.array_equal(fa.filter_dict[k], fb.filter_dict[k]), k
    assert (fa.boxes is None) == (fb.boxes is None)
    if fa.boxes is not None:
        assert np.array_equal(fa.boxes, fb.boxes, equal_nan=True)
    assert set(fa.cls) == set(fb.cls)
    for key in fa.cls:
        for f in fa.cls[key]:
            assert np.array_equal(fa.cls[key][f], fb.cls[key][f]), (key, f)
    assert set(ra) == set(rb)
    for k in ra:
        assert ra[k].dtype == rb[k].dtype and np.array_equal(ra[k], rb[k]), k
    if pa is not None:
        assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy())
