"""`min_samples` (and with it `clustering.model.min_cluster_size`) above 15: exact core distances for 16 <= k <= 64 on the GPU
(csrc/cluster_core.inc: k_cl_core_blk with its LDS-heap list and the wave-wide form of k_cl_core_far), through the C ABI, `HDBSCAN`, the fused pipeline and the CLI.

CPU: the oracle stays pinned to scikit-learn for the new range (MST weights bit-identical, tree stages equal on the same linkage);
the header's VG_CLUSTER_MAX_K.  GPU: squared core distances, MST, labels and probabilities equal to the oracle bit for bit.
The end-to-end adjusted-Rand condition of test_cluster.test_oracle_pinned_to_sklearn is not repeated here: equal-weight MST edges
are ordered arbitrarily by both libraries, and at k = 16 on the lidar scene scikit-learn against the oracle reads 0.9535."""
import ctypes
import functools
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import hdbscan_oracle as ho
from test_cluster import blob_scene, lidar_scene

PAIRS = [(15, 16), (15, 32), (25, 25), (40, 64), (10, 48)]            # (min_cluster_size, k = min_samples)
KS = (16, 17, 31, 32, 33, 48, 63, 64)
SMALL_KS = (1, 8)                                                     # the register list's own convention: the query is entry 0
SMALL_K_SCENES = ('blob', 'coincident', 'isolated', 'cell3000')
EPS = 0.15


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == 'lidar4k':
        return lidar_scene(1, 4000)
    if name == 'lidar5k':
        return lidar_scene(2, 5000)
    if name == 'lidar40k':
        return lidar_scene(7, 40000)
    assert name == 'blob'
    return blob_scene(0)


@functools.lru_cache(maxsize=None)
def _oracle_mst(name, k):
    X = _scene(name)
    core2 = ho.core_distances_sq(X, k)
    edges, w2 = ho.mst_prim(X, core2)
    e, w2s = ho.sort_edges(edges, w2)
    return core2, e, w2s


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('scene', ['lidar4k', 'blob'])
@pytest.mark.parametrize('mcs,k', PAIRS)
def test_oracle_pinned_to_sklearn_above_15(scene, mcs, k):
    from sklearn.cluster import HDBSCAN
    from sklearn.cluster._hdbscan import _tree
    from sklearn.cluster._hdbscan._linkage import HIERARCHY_dtype
    X = _scene(scene)
    n = len(X)
    # scikit-learn counts the point itself: its min_samples = k + 1
    m = HDBSCAN(min_cluster_size=mcs, min_samples=k + 1, cluster_selection_epsilon=EPS, algorithm='kd_tree').fit(X.astype(np.float64))
    _, e, w2s = _oracle_mst(scene, k)
    assert np.array_equal(np.sort(m._single_linkage_tree_['value']), np.sqrt(w2s))
    l, r, v, s = ho.single_linkage(e, np.sqrt(w2s), n)
    mine = np.zeros(n - 1, dtype=HIERARCHY_dtype)
    mine['left_node'], mine['right_node'], mine['value'], mine['cluster_size'] = l, r, v, s
    lab_sk, prob_sk = _tree.tree_to_labels(mine, mcs, 'eom', False, EPS, None)
    lab, prob = ho.tree_from_mst(e, w2s, n, mcs, EPS)
    assert np.array_equal(ho.canonical(lab), ho.canonical(lab_sk))
    print(f'{scene} mcs={mcs} k={k}: clusters {lab.max() + 1}, max |dp| {np.abs(prob - prob_sk).max()}')
    assert np.abs(prob - prob_sk).max() < 1e-12


def test_header_declares_max_k_and_library_exports_the_header():
    from vilgod_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'vilgod_hip.h')).read()
    assert int(re.search(r'#define\s+VG_CLUSTER_MAX_K\s+(\d+)', src).group(1)) == 64
    assert _lib.CLUSTER_MAX_K == 64
    declared = set()
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        declared |= set(_lib.parse_header(h).keys())
    assert {'vg_cluster_mst', 'vg_cluster_mst_nd'} <= declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in sorted(declared) if not hasattr(lib, n)]


def test_new_core_distance_kernels_use_no_scratch():
    from vilgod_amd import build
    text = build._device_asm('cluster.hip')
    sizes = dict(re.findall(r'\.set (\S+)\.private_seg_size, (\d+)', text))
    # the mangled name of every form: phase A with the register list, the LDS heap of 32 and of 64, phase B over 16 lanes and over the wave
    forms = {'register A': r'k_cl_core_blkILi\dE9ClRegList', 'heap-32 A': r'k_cl_core_blkILi\dE9ClLdsHeapILi32E',
             'heap-64 A': r'k_cl_core_blkILi\dE9ClLdsHeapILi64E', 'narrow B': r'k_cl_core_farILi\dELb0E', 'wide B': r'k_cl_core_farILi\dELb1E'}
    for form, pat in forms.items():
        names = {n for n in sizes if re.search(pat, n)}
        assert len(names) >= 3, (form, names)                        # DIM 3, 4, 5 are in the device code
        assert all(int(sizes[n]) == 0 for n in names), (form, {n: sizes[n] for n in names})
    assert build.check_scratch('cluster.hip', 'k_cl_core_blk') == [] and build.check_scratch('cluster.hip', 'k_cl_core_far') == []


def test_product_library_holds_one_walk_per_dim_and_no_development_kernel():
    from vilgod_amd import build
    text = build._device_asm('cluster.hip')
    vgprs = {n: int(v) for n, v in re.findall(r'\.set (\S+)\.num_vgpr, (\d+)', text)}
    kernels = {n for n in vgprs if 'k_cl_' in n}
    assert len(kernels) >= 40, sorted(kernels)                       # the names were found at all
    # the Boruvka walk: DIM 3, 4, 5 in workgroups of 512 threads, nothing else (mangled: k_cl_b_searchILi<DIM>ELi<NT>E...)
    walks = {n for n in kernels if re.match(r'_Z\d+k_cl_b_searchI', n)}
    assert sorted(re.match(r'_Z\d+k_cl_b_searchI(.*?)Ev', n).group(1) for n in walks) == ['Li3ELi512E', 'Li4ELi512E', 'Li5ELi512E'], walks
    # a 512-thread workgroup is two waves per SIMD: 256 registers each
    print({n: vgprs[n] for n in sorted(walks)})
    assert all(vgprs[n] <= 256 for n in walks), {n: vgprs[n] for n in walks}
    # what the development build alone has: the cooperative search that was retired, the per-point k-NN walk (k_cl_core itself, not
    # k_cl_core_blk / k_cl_core_far), the seeding simulation
    assert not [n for n in kernels if re.match(r'_Z\d+(k_cl_b_search_blk|k_cl_coreI|k_cl_seedsim_drop)', n)]
    assert build.check_scratch('cluster.hip', 'k_cl_') == []


# ------------------------------------------------------------------------------------------- GPU
def _model(cuda, n, mcs=15, k=None, hierarchy='host'):
    from vilgod_amd.hdbscan import HDBSCAN
    return HDBSCAN(cluster_selection_epsilon=EPS, min_cluster_size=mcs, min_samples=k, metric='euclidean', core_dist_n_jobs=-1,
                   max_points=n + 16, device=cuda, hierarchy=hierarchy)


@pytest.mark.gpu
def test_min_cluster_size_20_constructs_and_fits_and_65_is_refused(cuda):
    from vilgod_amd.hdbscan import HDBSCAN
    X = _scene('blob')
    m = HDBSCAN(min_cluster_size=20, cluster_selection_epsilon=EPS, max_points=len(X) + 16, device=cuda)
    assert m.min_samples == 20
    m.fit(X)
    want_l, want_p = ho.fit(X, 20, EPS)
    assert np.array_equal(m.labels_, want_l) and np.array_equal(m.probabilities_, want_p)
    with pytest.raises(NotImplementedError, match='64'):
        HDBSCAN(min_samples=65, device=cuda)
    with pytest.raises(NotImplementedError, match='64'):
        HDBSCAN(min_cluster_size=65, device=cuda)
    HDBSCAN(min_cluster_size=65, min_samples=64, max_points=1000, device=cuda)        # only min_samples is bounded


@pytest.mark.gpu
def test_c_abi_accepts_1_to_max_k_only(cuda):
    import torch
    from vilgod_amd._lib import lib, ptr, stream_ptr
    X = torch.from_numpy(_scene('blob')[:500]).to(cuda)
    n = X.shape[0]
    h = ctypes.c_void_p()
    assert lib.vg_cluster_create(ctypes.byref(h), 1000) == 0
    try:
        lo = torch.empty(n - 1, dtype=torch.int32, device=cuda)
        hi = torch.empty(n - 1, dtype=torch.int32, device=cuda)
        w2 = torch.empty(n - 1, dtype=torch.float64, device=cuda)
        for k, want in ((0, 1), (1, 0), (64, 0), (65, 1), (1000, 1)):
            rc = lib.vg_cluster_mst_nd(h, ptr(X), n, X.stride(0), 3, k, None, ptr(lo), ptr(hi), ptr(w2), None, stream_ptr())
            assert rc == want, (k, rc)
    finally:
        lib.vg_cluster_destroy(h)


def _nd(X3, dim, seed=0):
    """columns 4 / 5 of the two-frame clustering input: an entropy score in [0, 1] and 0.1 x frame number (0 or 1)"""
    rng = np.random.default_rng(seed)
    n = len(X3)
    cols = [X3[:, :3].astype(np.float32)]
    if dim >= 4:
        cols.append(rng.uniform(0, 1, (n, 1)).astype(np.float32))
    if dim >= 5:
        cols.append((np.float32(0.1) * rng.integers(0, 2, (n, 1)).astype(np.float32)).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(cols, 1), np.float32)


def _stress_scene(name, k):
    rng = np.random.default_rng(11)
    if name == 'n_le_k':                       # fewer than k other points: every core distance is +inf
        return rng.normal(size=(k, 3)).astype(np.float32)
    if name == 'n_k_plus_1':                   # exactly k others: every list is full at the very end
        return (rng.normal(size=(k + 1, 3)) * 2).astype(np.float32)
    if name == 'coincident':                   # distance ties (0 and equal non-zero distances) at the k-th place
        cloud = rng.normal(size=(600, 3)) * 0.5
        return np.concatenate([cloud, np.repeat(cloud[:1], 199, 0), np.repeat([[4.0, 0.0, 0.0]], 70, 0)]).astype(np.float32)
    if name == 'isolated':                     # 64 points 30 m apart beside a dense blob: their neighbours are far outside any shell
        gx, gy = np.meshgrid(np.arange(8) * 30.0, np.arange(8) * 30.0)
        iso = np.stack([gx.ravel(), gy.ravel(), np.zeros(64)], 1)
        blob = rng.normal(size=(2000, 3)) * 0.3 + [-25.0, -25.0, 0.0]
        return np.concatenate([iso, blob]).astype(np.float32)
    assert name == 'cell3000'                  # one 0.4 m cell with 3 000 points: level-0 work items cut into chunks of 64
    dense = rng.uniform(0, 0.1, size=(3000, 3)) + [3.0, 3.0, 0.5]
    around = rng.uniform(-10, 10, size=(400, 3)) * [1, 1, 0.1]
    return np.concatenate([dense, around]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [3, 4, 5])
@pytest.mark.parametrize('scene', ['lidar5k', 'lidar40k', 'blob', 'n_le_k', 'n_k_plus_1', 'coincident', 'isolated', 'cell3000'])
def test_core_distances_equal_oracle(cuda, scene, dim):
    """k <= 15 runs the register list and the 16-lane phase B (asserted next to the other cases: a dispatch slip shows here),
    the others the LDS heap and the wave-wide phase B."""
    import torch
    for k in (SMALL_KS if scene in SMALL_K_SCENES else ()) + (15,) + KS:
        X3 = _scene(scene) if scene in ('lidar5k', 'lidar40k', 'blob') else _stress_scene(scene, k)
        X = _nd(X3, dim)
        n = len(X)
        model = _model(cuda, n, 15, k)
        _, _, _, core2 = model.mst(torch.from_numpy(X).to(cuda), want_core=True, dim=dim)
        core2 = core2.cpu().numpy()
        want = ho.core_distances_sq(X, k)
        bad = np.flatnonzero(core2 != want)
        assert bad.size == 0, (scene, dim, k, bad.size, bad[:5], core2[bad[:5]], want[bad[:5]])
        if scene == 'n_le_k':
            assert np.isinf(core2).all()
        else:
            assert np.isfinite(core2).all()


@pytest.mark.gpu
@pytest.mark.parametrize('scene', ['lidar4k', 'blob'])
@pytest.mark.parametrize('mcs,k', PAIRS)
def test_mst_and_labels_equal_oracle(cuda, scene, mcs, k):
    import torch
    X = _scene(scene)
    n = len(X)
    want_core2, e, w2s = _oracle_mst(scene, k)
    model = _model(cuda, n, mcs, k)
    lo, hi, w2, core2 = model.mst(torch.from_numpy(X).to(cuda), want_core=True)
    lo, hi, w2, core2 = lo.cpu().numpy(), hi.cpu().numpy(), w2.cpu().numpy(), core2.cpu().numpy()
    assert np.array_equal(core2, want_core2)
    assert np.array_equal(w2, w2s)                                   # weights, sorted
    got = np.stack([lo, hi], 1)[np.lexsort((hi, lo, w2))]
    assert np.array_equal(got, e)                                    # the same (unique) tree
    want_l, want_p = ho.tree_from_mst(e, w2s, n, mcs, EPS)
    for hierarchy in ('host', 'device'):
        m = _model(cuda, n, mcs, k, hierarchy)
        assert m.hierarchy == ('host' if mcs > 32 else hierarchy)    # the device stage holds min_cluster_size <= 32
        m.fit(X)
        assert np.array_equal(m.labels_, want_l), hierarchy
        assert np.array_equal(m.probabilities_, want_p), hierarchy
    print(f'{scene} mcs={mcs} k={k}: n={n} clusters={want_l.max() + 1} rounds={model.n_rounds_}')


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [4, 5])
def test_two_frame_input_labels_equal_oracle(cuda, dim):
    """the 4-/5-D clustering space with min_cluster_size = 20 (= min_samples): labels through `fit` like the two-frame stage"""
    X = _nd(_scene('blob'), dim, seed=3)
    for hierarchy in ('host', 'device'):
        m = _model(cuda, len(X), 20, None, hierarchy).fit(X)
        wl, wp = ho.fit(X, 20, EPS)
        assert np.array_equal(ho.canonical(m.labels_), ho.canonical(wl)) and np.array_equal(m.probabilities_, wp)


@pytest.mark.gpu
def test_pipeline_with_min_cluster_size_20_in_both_pack_modes(cuda):
    from oracle import segment_oracle as so
    from test_pack_device import _pair, _same_frame
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['clustering']['model']['min_cluster_size'] = 20
    host, dev = _pair(cuda, cfg, vit_dtype='f32', max_points=25_000, angle_mode='reference')
    assert host.cluster_model.min_samples == 20 and dev.cluster_model.min_cluster_size == 20
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fa, ra = host.process_frame(pts, poses[1], poses[0], fnr=1)
    pa = host.last_probs
    fb, rb = dev.process_frame(pts, poses[1], poses[0], fnr=1)
    assert fa.n_detections > 5 and fa.valid.sum() > 2
    _same_frame(fa, ra, pa, fb, rb, dev.last_probs)
    gm = np.zeros(len(pts), bool)
    gm[fa.ground_point_indices] = True
    X = so.apply_transform(pts, fa.transform_to_ref)[~gm][:, :3]
    labels, probs = ho.fit(X, 20, EPS)
    dets = so.generate_detections(labels, probs)                     # the probability cut of the reference
    for fs in (fa, fb):
        assert [int(c) for c in fs.cluster_ids] == [c for c, _ in dets]
        for c, (_, idx) in enumerate(dets):
            assert np.array_equal(fs.cluster_index(c), idx)


@pytest.mark.gpu
def test_two_frame_sequence_with_min_cluster_size_20_in_both_pack_modes(cuda):
    from test_pack_device import _pair, _same_frame
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['clustering']['model']['min_cluster_size'] = 20
    host, dev = _pair(cuda, cfg, vit_dtype='f16', max_points=25_000)
    frames, poses = synthetic.make_sequence(seed=2, n_frames=4, n_points=12_000, n_objects=8)
    ent_args = dict(n_neighbouring_frames=3, skip_frames=0)
    a = host.process_sequence(frames, poses, poses[0], entropy_args=ent_args, n_frames=2, seed=0)
    b = dev.process_sequence(frames, poses, poses[0], entropy_args=ent_args, n_frames=2, seed=0)
    assert sum(int(fa.n_detections) for fa, _ in a) > 5
    for (fa, ra), (fb, rb) in zip(a, b):
        _same_frame(fa, ra, None, fb, rb, None)


@pytest.mark.gpu
def test_cli_with_min_cluster_size_20(cuda, tmp_path):
    root = str(tmp_path / 'mcs20')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'preprocess_data.py'), 'preprocessor=waymo',
                        'preprocessor.clustering.model.min_cluster_size=20', f'dataset.DATA_PATH={root}',
                        'dataset.SYNTHETIC.frames_per_sequence=6', 'dataset.SYNTHETIC.points_per_frame=12000',
                        'dataset.SYNTHETIC.objects_per_frame=8', 'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0',
                        'device.max_points=16000', 'paths.clip_model=/nonexistent'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = glob.glob(f'{root}/preprocessed_data/results/vilgod_mi355x/*/synthetic_train_0000.pkl')
    seq = glob.glob(f'{root}/preprocessed_data/vilgod_mi355x_seq/synthetic_train_0000.pkl')
    assert len(res) == 1 and len(seq) == 1
    import pickle
    with open(res[0], 'rb') as f:
        out = pickle.load(f)
    with open(seq[0], 'rb') as f:
        state = pickle.load(f)
    assert len(out) == 6 and len(state) == 6
    assert sum(len(st['_detections']) for st in state) > 0
