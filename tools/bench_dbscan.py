"""DBSCAN on the benchmark's frame: vg_cluster_dbscan beside what a user would trade it against, HDBSCAN's mst() + tree_device on the
same points, and scikit-learn's DBSCAN where it imports.  One JSON line (also written to --json, default profiles/dbscan_bench.json):

    python tools/bench_dbscan.py [--points 150000] [--eps 0.3 0.5 1.0] [--min-samples 5 10 15] [--reps 20] [--rounds 5] [--json ...]

Workload: the non-ground points of bench.py's first frame (synthetic.make_frame(1, 150 000 points, 60 objects); ground from the
pipeline's own segmentation: about 79 k points stay), x, y, z, in input order (`input`) and in `entropy.spatial_order` (`spatial`).
  dbscan_gpu_ms    one vg_cluster_dbscan call (grid build included: it is part of the call), between two HIP events: ms per call
  dbscan_ms        the same calls, wall time with the stream drained at the end
  clusters, core, noise   what the call found (equal in both orders up to the numbering; asserted)
  hdbscan          HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15, hierarchy='device'): mst() + tree_device per call, wall
                   time with the stream drained (mst() waits for its rounds itself) -- the shipped configuration's front stage
  sklearn_ms       sklearn.cluster.DBSCAN(eps, min_samples, n_jobs=16).fit on the float64 copy of the `input` array, timed ONCE per
                   setting; labels and core samples compared with the device's (`sklearn_equal`); absent when scikit-learn is not importable
10 warm-up calls, then the median of `rounds` measurements of `reps` calls with their min and max.
Not measured here: real frames, a captured graph's replay time, several frames in flight, dim 5.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_knn import _measure, _stats, nonground      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--eps', type=float, nargs='*', default=[0.3, 0.5, 1.0])
    ap.add_argument('--min-samples', type=int, nargs='*', default=[5, 10, 15])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'dbscan_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import synthetic
    from vilgod_amd.dbscan import DBSCAN
    from vilgod_amd.entropy import spatial_order
    from vilgod_amd.hdbscan import HDBSCAN
    from vilgod_amd.pipeline import PseudoLabelPipeline
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent')
    X = nonground(pipe, synthetic, 1, a.points, a.objects, synthetic.make_poses(2))
    del pipe
    n = len(X)
    d_in = torch.from_numpy(X).to(dev)
    d_sp = d_in.index_select(0, spatial_order(d_in)).contiguous()
    res = {'metric': 'dbscan_ms', 'points': a.points, 'nonground': n, 'reps': a.reps, 'rounds': a.rounds, 'settings': []}
    sk = None
    if not a.no_sklearn:
        try:
            from sklearn.cluster import DBSCAN as sk
        except ImportError:
            sk = None
    for eps in a.eps:
        for ms in a.min_samples:
            model = DBSCAN(eps=eps, min_samples=ms, max_points=n)
            row = {'eps': eps, 'min_samples': ms}
            found = {}
            for name, d_X in (('input', d_in), ('spatial', d_sp)):
                call = lambda: model.labels_device(d_X)
                row[name] = {'dbscan_gpu_ms': _measure(call, a.reps, a.rounds, events=True), 'dbscan_ms': _measure(call, a.reps, a.rounds)}
                lab, _, nc, core = model.labels_device(d_X)
                found[name] = (int(nc.item()), int(core.sum().item()), int((lab < 0).sum().item()))
            assert found['input'] == found['spatial'], found
            row['clusters'], row['core'], row['noise'] = found['input']
            if sk is not None:
                t0 = time.perf_counter()
                m = sk(eps=eps, min_samples=ms, n_jobs=16).fit(X.astype(np.float64))
                row['sklearn_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
                lab, _, _, core = model.labels_device(d_in)
                row['sklearn_equal'] = bool(np.array_equal(lab.cpu().numpy(), m.labels_) and
                                            np.array_equal(np.flatnonzero(core.cpu().numpy()), m.core_sample_indices_))
            del model
            res['settings'].append(row)
    hd = HDBSCAN(min_cluster_size=15, cluster_selection_epsilon=0.15, max_points=n, hierarchy='device')
    res['hdbscan'] = {}
    for name, d_X in (('input', d_in), ('spatial', d_sp)):
        def front():
            lo, hi, w2 = hd.mst(d_X)
            return hd.tree_device(lo, hi, w2, n)
        res['hdbscan'][name] = {'mst_tree_ms': _measure(front, a.reps, a.rounds), 'mst_ms': _measure(lambda: hd.mst(d_X), a.reps, a.rounds)}
    res['sklearn'] = sk is not None
    res['device'] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
