"""DBSCAN without a GPU: the contract (tests/dbscan_ref.py) against scikit-learn's recorded results, vg_dbscan_host against the contract,
the refusals, the Python class's argument handling and the pipeline's `_target_` dispatch.

Every comparison is exact.  The fixture (tests/golden/make_dbscan.py) holds scikit-learn's labels_ and core_sample_indices_; the
conditions on its inputs that make those independent of scikit-learn's own rounding are re-asserted here.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_dbscan as mk      # noqa: E402
import dbscan_ref as dr      # noqa: E402

ORDERS = ('built', 'reversed', 'shuffled')


class Scenes:
    """the fixture, loaded once: scene k -> (meta, X, sklearn labels, sklearn core indices)"""

    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, 'dbscan_golden.npz'))
        self.meta = json.loads(str(self.z['meta']))
        self.names = [m['name'] for m in self.meta]

    def __call__(self, name):
        k = self.names.index(name)
        m = self.meta[k]
        X = self.z[f'X_{k}'].reshape(-1, m['dim']) if f'X_{k}' in self.z else mk.kitti_rows()
        return m, X, self.z[f'labels_{k}'], self.z[f'core_{k}']


SCENES = Scenes()
SMALL = [n for n in SCENES.names if n != 'kitti_20000']


def host(X, eps, ms, dim=None):
    from vilgod_amd.dbscan import dbscan_host
    return dbscan_host(X, eps, ms, dim)


def test_the_fixture_is_the_scene_list():
    """the maker's scenes are what the file holds (a changed maker without a regenerated file is caught here)"""
    built = mk.scenes()
    assert [s['name'] for s in built] + ['kitti_20000'] == SCENES.names
    for s in built:
        m, X, _, _ = SCENES(s['name'])
        assert np.array_equal(X, s['X']) and (m['eps'], m['min_samples'], m['dim']) == (s['eps'], s['min_samples'], s['dim'])


@pytest.mark.parametrize('name', SCENES.names)
def test_input_conditions(name):
    """margins, exact lattices, shared border rows, border-first clusters: conditions on the inputs, not measurements"""
    m, X, _, _ = SCENES(name)
    mk.check_inputs(m, X)


@pytest.mark.parametrize('name', SMALL)
def test_contract_equals_sklearn(name):
    m, X, labels, core = SCENES(name)
    rl, rc, nc = dr.dbscan_ref(X, m['eps'], m['min_samples'])
    assert np.array_equal(rl, labels) and np.array_equal(np.flatnonzero(rc), core)
    assert nc == (labels.max() + 1 if labels.size else 0)


@pytest.mark.parametrize('name', SMALL)
def test_host_equals_contract(name):
    m, X0, _, _ = SCENES(name)
    for order in ORDERS:
        X = dr.reorder(X0, order)
        rl, rc, rn = dr.dbscan_ref(X, m['eps'], m['min_samples'])
        hl, hc, hp, hn = host(X, m['eps'], m['min_samples'])
        assert np.array_equal(hl, rl) and np.array_equal(hc.astype(bool), rc) and hn == rn, order
        assert np.array_equal(hp, (rl >= 0).astype(np.float64)), order
        if X.shape[0] < 2:
            break


def test_host_equals_sklearn_on_the_real_frame():
    m, X, labels, core = SCENES('kitti_20000')
    hl, hc, hp, hn = host(X, m['eps'], m['min_samples'])
    assert np.array_equal(hl, labels) and np.array_equal(np.flatnonzero(hc), core) and hn == labels.max() + 1
    assert np.array_equal(hp, (labels >= 0).astype(np.float64))


def test_dim_decides():
    """identical x, y, z, more than eps apart in the 4th coordinate: two clusters at dim 4, one at dim 3 of the SAME array"""
    m, X, _, _ = SCENES('dim4_two_groups')
    assert host(X, m['eps'], m['min_samples'], 4)[3] == 2
    assert host(X, m['eps'], m['min_samples'], 3)[3] == 1


def test_inclusive_threshold_flips():
    m7, X, l7, _ = SCENES('lattice_ms7')
    _, _, l8, _ = SCENES('lattice_ms8')
    assert (l7 >= 0).any() and (l8 < 0).all()                       # interior rows have exactly 7 neighbours
    _, _, lb, _ = SCENES('lattice_below_ms2')
    assert (lb < 0).all()                                            # one step below 0.5 nothing is a neighbour of anything else


def test_kernels_are_built_for_the_device_and_do_not_spill():
    import re
    from vilgod_amd import build, _lib
    asm = build._device_asm('cluster.hip')
    for k in ('k_db_core', 'k_db_union', 'k_db_roots', 'k_db_mark', 'k_db_label', 'k_db_border', 'k_cl_grid_reset'):
        assert re.search(r'^_Z\S*' + k + r'\S*:', asm, flags=re.M), k
    assert build.check_scratch('cluster.hip', 'k_db_') == []
    for m in re.finditer(r'\.amdhsa_kernel (\S*k_db_\S*)(.*?)\.end_amdhsa_kernel', asm, flags=re.S):
        assert re.search(r'\.amdhsa_group_segment_fixed_size 0\b', m.group(2)), m.group(1)      # no LDS either
    protos = _lib.parse_header()
    assert [a for _, a in protos['vg_cluster_dbscan'][1]] == ['h', 'd_points', 'n', 'stride', 'dim', 'eps', 'min_samples', 'd_labels', 'd_core',
                                                             'd_probs', 'd_n_clusters', 'stream']
    assert [a for _, a in protos['vg_dbscan_host'][1]] == ['h_points', 'n', 'stride', 'dim', 'eps', 'min_samples', 'h_labels', 'h_core', 'h_probs',
                                                          'h_n_clusters']
    assert _lib.lib.vg_abi_version() == 2                           # an addition: the version stays


# ================================================================================================ refusals
def _raw_host(X, n, stride, dim, eps, ms, null=()):
    from vilgod_amd._lib import lib
    labels, core, probs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.float64)
    nc = ctypes.c_int32(-7)
    p = lambda a, key: None if key in null else a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.vg_dbscan_host(p(X, 'X'), n, stride, dim, eps, ms, p(labels, 'labels'), p(core, 'core'), p(probs, 'probs'),
                            None if 'nc' in null else ctypes.byref(nc))
    return rc, nc.value


def test_c_refusals():
    X = np.zeros((4, 5), np.float32)
    ok = dict(n=4, stride=5, dim=3, eps=0.5, ms=2)
    assert _raw_host(X, **ok) == (0, 1)
    for bad in (dict(eps=float('nan')), dict(eps=0.0), dict(eps=-1.0), dict(eps=np.nextafter(3.2, 4)), dict(eps=float('inf')), dict(ms=0),
                dict(ms=-3), dict(dim=2), dict(dim=6), dict(n=-1), dict(stride=2), dict(dim=5, stride=4)):
        rc, nc = _raw_host(X, **{**ok, **bad})
        assert rc == 1, bad
    assert _raw_host(X, **{**ok, 'eps': 3.2})[0] == 0               # the limit itself: ceil(3.2 / 0.4) == 8
    assert _raw_host(X, **ok, null=('probs',)) == (0, 1)             # probabilities are optional
    for key in ('X', 'labels', 'core', 'nc'):
        assert _raw_host(X, **ok, null=(key,))[0] == 1, key
    assert _raw_host(X, **{**ok, 'n': 0}, null=('X', 'labels', 'core')) == (0, 0)      # n == 0: VG_OK, no clusters


def test_python_refusals():
    from vilgod_amd.dbscan import DBSCAN
    for eps in (float('nan'), 0.0, -0.5, 3.3, float('inf')):
        with pytest.raises(ValueError, match=r'eps.*3\.2 m'):
            DBSCAN(eps=eps)
    for ms in (0, -1, 2.5):
        with pytest.raises(ValueError, match='min_samples'):
            DBSCAN(min_samples=ms)
    with pytest.raises(NotImplementedError):
        DBSCAN(metric='manhattan')
    with pytest.raises(TypeError, match='cluster_selection_epsilon'):
        DBSCAN(cluster_selection_epsilon=0.15)


def test_target_dispatch():
    from vilgod_amd.pipeline import cluster_model_spec, default_preprocessor_cfg
    from vilgod_amd.dbscan import DBSCAN
    from vilgod_amd.hdbscan import HDBSCAN
    for target in ('sklearn.cluster.DBSCAN', 'vilgod_amd.dbscan.DBSCAN', 'DBSCAN'):
        cls, kw = cluster_model_spec({'_target_': target, 'eps': 0.7, 'min_samples': 4}, hierarchy='host')
        assert cls is DBSCAN and kw == {'eps': 0.7, 'min_samples': 4}          # no hierarchy key: DBSCAN has no such stage
    for target in ('hdbscan.HDBSCAN', 'vilgod_amd.hdbscan.HDBSCAN', 'sklearn.cluster.HDBSCAN', 'sklearn.cluster.OPTICS', None):
        cfg = {'min_cluster_size': 15}
        if target is not None:
            cfg['_target_'] = target
        cls, kw = cluster_model_spec(cfg, hierarchy='host')
        assert cls is HDBSCAN and kw == {'min_cluster_size': 15, 'hierarchy': 'host'}
    ccfg = default_preprocessor_cfg()['clustering']
    cls, kw = cluster_model_spec(ccfg['model'])
    assert cls is HDBSCAN and kw['min_cluster_size'] == 15 and kw['hierarchy'] in ('host', 'device')
    with pytest.raises(ValueError):
        cluster_model_spec({'min_cluster_size': 15}, hierarchy='gpu')


def test_shipped_config_names_dbscan():
    from vilgod_amd.pipeline import cluster_model_spec
    from vilgod_amd.dbscan import DBSCAN
    import yaml
    from conftest import ROOT
    with open(os.path.join(ROOT, 'tools', 'configs', 'preprocessor', 'waymo_dbscan.yaml')) as f:
        cfg = yaml.safe_load(f)
    cls, kw = cluster_model_spec(cfg['clustering']['model'])
    assert cls is DBSCAN and kw == {'eps': 0.5, 'min_samples': 10}
    with open(os.path.join(ROOT, 'tools', 'configs', 'preprocessor', 'waymo.yaml')) as f:
        ref = yaml.safe_load(f)
    cfg['clustering'].pop('model'), ref['clustering'].pop('model')
    assert cfg == ref                                                # waymo.yaml in everything but the model
    # the CLI's loader resolves the choice, its dataset file included (the data of preprocessor=waymo)
    from vilgod_amd import config as vconfig
    job = vconfig.load(os.path.join(ROOT, 'tools', 'configs'), 'preprocessing', ['preprocessor=waymo_dbscan'])
    way = vconfig.load(os.path.join(ROOT, 'tools', 'configs'), 'preprocessing', ['preprocessor=waymo'])
    assert dict(job.preprocessor.clustering.model) == {'_target_': 'vilgod_amd.dbscan.DBSCAN', 'eps': 0.5, 'min_samples': 10}
    assert job.dataset.DATASET_TARGET == way.dataset.DATASET_TARGET and dict(job.dataset.SYNTHETIC) == dict(way.dataset.SYNTHETIC)


# ================================================================================================ fresh seeds against scikit-learn
def test_fresh_seeds_against_sklearn():
    sk = pytest.importorskip('sklearn.cluster')
    done = 0
    for seed in range(1000, 1060):                                   # none of these is in the fixture
        X, eps, ms, lattice = dr.random_scene(seed)
        if not lattice and not dr.margin(X, eps) > 1e-9:
            continue
        m = sk.DBSCAN(eps=eps, min_samples=ms).fit(X.astype(np.float64))
        rl, rc, _ = dr.dbscan_ref(X, eps, ms)
        hl, hc, _, _ = host(X, eps, ms)
        assert np.array_equal(rl, m.labels_) and np.array_equal(np.flatnonzero(rc), m.core_sample_indices_), seed
        assert np.array_equal(hl, m.labels_) and np.array_equal(np.flatnonzero(hc), m.core_sample_indices_), seed
        done += 1
    assert done >= 55
