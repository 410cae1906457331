"""The DBSCAN model inside the pipeline: `clustering.model._target_` builds it, `cluster()` is one queued call equal to the host twin,
`label` runs on its labels in both pack modes, the two-frame clusterer takes its 5-D branch, and the CLI runs `preprocessor=waymo_dbscan`.
"""
import logging
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from vilgod_amd import synthetic

pytestmark = pytest.mark.gpu

MODEL = {'_target_': 'sklearn.cluster.DBSCAN', 'eps': 0.5, 'min_samples': 10}


def _cfg():
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['clustering']['model'] = dict(MODEL)
    return cfg


@pytest.fixture(scope='module')
def pipes(cuda):
    """the 20k-point frame's two pipelines (pack='host' and 'device', one tower), built once"""
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from vilgod_amd.dbscan import DBSCAN
    kw = dict(device=cuda, vit_dtype='f32', max_points=25_000, clip_model_path='/nonexistent', angle_mode='reference')
    host = PseudoLabelPipeline(_cfg(), hierarchy='host', **kw)                     # (hierarchy= is ignored for this model)
    dev = PseudoLabelPipeline(_cfg(), clip=host.clip, pack='device', **kw)
    for p in (host, dev):
        assert isinstance(p.cluster_model, DBSCAN) and p.hierarchy is None
        assert (p.cluster_model.eps, p.cluster_model.min_samples, p.cluster_model.max_points) == (0.5, 10, 25_000)
    assert isinstance(host._clone_for_worker().cluster_model, DBSCAN)              # worker copies follow the same rule
    return host, dev


def test_cluster_equals_the_host_twin(pipes, cuda):
    from vilgod_amd.dbscan import dbscan_host
    host, dev = pipes
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fs, d_ref, d_X, gidx = host.prepare(pts, poses[1], poses[0], fnr=1)
    want_l, _, want_p, want_n = dbscan_host(d_X.cpu().numpy()[:, :3], 0.5, 10)
    assert want_n > 5
    host._lat = {'_t': 0.0}
    try:
        labels, probs = host.cluster(d_X)
        assert 'dbscan_kernels' in host._lat and 'mst_kernels' not in host._lat
    finally:
        host._lat = None
    assert isinstance(labels, np.ndarray) and np.array_equal(labels, want_l) and np.array_equal(probs, want_p)
    d_labels, d_probs = dev.cluster(d_X)
    assert d_labels.is_cuda and d_probs.is_cuda and d_labels.dtype == torch.int32 and d_probs.dtype == torch.float64
    assert np.array_equal(d_labels.cpu().numpy(), want_l) and np.array_equal(d_probs.cpu().numpy(), want_p)
    assert dev.cluster_model.label_bound(7) == 8 and dev.pack_device(d_labels, d_probs) is not None
    for n in (0, 1):                                                                 # an empty and a one-row frame: noise, no fault
        l, p = host.cluster(d_X[:n])
        assert l.shape == (n,) and (l < 0).all() and (p == 0).all()


def test_label_runs_and_both_pack_modes_leave_identical_states(pipes):
    from test_pack_device import _same_frame
    host, dev = pipes
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fa, ra = host.process_frame(pts, poses[1], poses[0], fnr=1)
    pa = host.last_probs
    fb, rb = dev.process_frame(pts, poses[1], poses[0], fnr=1)
    assert set(ra) == {'boxes_lidar', 'name', 'score', 'moving'} and ra['boxes_lidar'].shape[1] == 7
    assert fa.n_detections > 5 and fa.valid.sum() > 2 and len(ra['name']) > 0
    _same_frame(fa, ra, pa, fb, rb, dev.last_probs)


def test_two_frame_clusterer_equals_host_twin_plus_nearest(cuda):
    from vilgod_amd.dbscan import DBSCAN, dbscan_host
    from vilgod_amd.entropy import EntropyScorer, TwoFrameClusterer, full_scores
    frames, _ = synthetic.make_sequence(seed=3, n_frames=3, n_points=9000, n_objects=12)
    d = [torch.from_numpy(np.ascontiguousarray(f[:, :3], dtype=np.float32)).to(cuda) for f in frames]
    model = DBSCAN(eps=0.5, min_samples=10, max_points=50_000, device=cuda)
    scorer = EntropyScorer(model, n_neighbouring_frames=2, skip_frames=0)
    H = scorer.score_sequence(d)
    ent = []
    for f in range(3):
        vals, idx = scorer.reduce(H[f])
        ent.append(full_scores(d[f].shape[0], vals, idx, device=cuda))
    two = TwoFrameClusterer(model, n_frames=2, seed=0)
    total = 0
    for fnr in range(3):
        seq = two.cluster_input(fnr, d, ent)
        assert seq.shape[1] == 5
        want_seq, _, want_pseq, _ = dbscan_host(seq.cpu().numpy(), 0.5, 10, 5)
        labels, probs = two.labels(fnr, d, ent)
        model.grid(seq)                                                              # the transfer, with the existing `nearest`
        idx, _ = model.nearest(d[fnr], two.gate)
        idx = idx.cpu().numpy().astype(np.int64)
        ok = idx >= 0
        want = np.where(ok, want_seq[np.maximum(idx, 0)], -1).astype(np.int64)
        assert labels.dtype == np.int64 and np.array_equal(labels, want)
        assert np.array_equal(probs, np.where(ok, want_pseq[np.maximum(idx, 0)], 0.0))
        total += int((labels >= 0).sum())
    assert total > 300


def test_cli_runs_the_dbscan_config(cuda, tmp_path, caplog):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    from test_cli import OVR, _load
    root = str(tmp_path / 'db')
    with caplog.at_level(logging.INFO):
        preprocess_data.main(['preprocessor=waymo_dbscan', f'dataset.DATA_PATH={root}'] + OVR)
    out, idx, state = _load(root)
    assert len(out) == 6 and idx == [0, 1, 2, 3, 4, 5] and len(state) == 6
    assert any(len(fr['name']) > 0 for fr in out)                                    # at least one frame has detections
    assert max(len(fr['name']) for fr in out) > 2
    assert any('Clustering model: DBSCAN(eps=0.5, min_samples=10)' in r.getMessage() for r in caplog.records)
