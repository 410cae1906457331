"""K nearest neighbours on the benchmark's frame: vg_cluster_knn beside vg_cluster_nearest, the numpy wrapper and scipy's KD-tree, one
JSON line (also written to --json, default profiles/knn_bench.json):

    python tools/bench_knn.py [--points 150000] [--K 1 4 8 16 32] [--reps 20] [--rounds 5] [--json profiles/knn_bench.json]

Workload: the non-ground points of bench.py's first frame (synthetic.make_frame(1, 150 000 points, 60 objects); ground from the
pipeline's own segmentation: about 79 k points stay), searched against themselves (`self`: every query is a target, K = 4 is
zero_shot_detector.py:221) and against the next frame's non-ground points (`next`: the label transfer's shape, :237).  The queries
are in `entropy.spatial_order`, as every caller in the package sends them; the grid is built once per target set, outside the timing.
  knn_gpu_ms     vg_cluster_knn, no gate, between two HIP events: ms per launch
  knn_ms         the same launches, wall time with the stream drained at the end
  gate           K = 1 with the 0.2 gate of knn_labels beside vg_cluster_nearest with the same gate (equal results asserted)
  numpy_ms       vilgod_amd.knn.knn numpy in, numpy out (upload, grid, order, launch, put back, download), K = 1 and 4
  ckdtree_ms     scipy.spatial.cKDTree(target).query(query, K, workers=16) on float64 copies, tree construction included once per
                 round; absent when scipy is not importable
10 warm-up launches, then the median of `rounds` measurements of `reps` launches with their min and max.
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


def _stats(v):
    return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4), 'max': round(float(max(v)), 4)}


def _measure(fn, reps, rounds, warmup=10, events=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        else:
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / reps)
    return _stats(out)


def nonground(pipe, synthetic, seed, points, objects, poses):
    """the frame's points without the ground the pipeline's own segmentation finds (float32 [m, 3], sensor frame)"""
    pts = synthetic.make_frame(seed, points, n_objects=objects)
    fs, _ = pipe.process_frame(pts, poses[1], poses[0], fnr=seed)
    torch.cuda.synchronize()
    keep = np.ones(len(pts), bool)
    keep[fs.ground_point_indices] = False
    return np.ascontiguousarray(pts[keep, :3], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--K', type=int, nargs='*', default=[1, 4, 8, 16, 32])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'knn_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import knn as vk, synthetic
    from vilgod_amd.entropy import spatial_order
    from vilgod_amd.hdbscan import HDBSCAN
    from vilgod_amd.pipeline import PseudoLabelPipeline
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent')
    poses = synthetic.make_poses(2)
    frames = [nonground(pipe, synthetic, s, a.points, a.objects, poses) for s in (1, 2)]
    del pipe
    model = HDBSCAN(max_points=max(len(f) for f in frames))
    gate = float(np.nextafter(np.float32(0.2), np.float32(0)))           # knn_labels: `dists > 0.2` in float64 on float32 distances
    res = {'metric': 'knn_ms', 'points': a.points, 'nonground': [len(f) for f in frames], 'reps': a.reps, 'rounds': a.rounds, 'cases': []}
    q_np = frames[0]
    d_q = torch.from_numpy(q_np).to(dev)
    d_q = d_q.index_select(0, spatial_order(d_q)).contiguous()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    for name, t_np in (('self', frames[0]), ('next', frames[1])):
        d_t = torch.from_numpy(t_np).to(dev)
        model.grid(d_t)
        case = {'targets': name, 'n_query': len(q_np), 'n_target': len(t_np), 'K': {}}
        for K in a.K:
            out = (torch.empty((len(q_np), K), dtype=torch.int32, device=dev), torch.empty((len(q_np), K), dtype=torch.float32, device=dev))
            call = lambda: model.knn(d_q, K, out=out)
            case['K'][str(K)] = {'knn_gpu_ms': _measure(call, a.reps, a.rounds, events=True), 'knn_ms': _measure(call, a.reps, a.rounds)}
        ki, kd = model.knn(d_q, 1, gate)
        ni, nd = model.nearest(d_q, gate)
        assert torch.equal(ki[:, 0], ni) and torch.equal(kd[:, 0], nd)
        out1 = (torch.empty_like(ki), torch.empty_like(kd))
        case['gate'] = {'max_d2': gate, 'found': round(float((ni >= 0).float().mean()), 4),
                        'knn_k1_gpu_ms': _measure(lambda: model.knn(d_q, 1, gate, out=out1), a.reps, a.rounds, events=True),
                        'nearest_gpu_ms': _measure(lambda: model.nearest(d_q, gate), a.reps, a.rounds, events=True)}
        case['numpy_ms'] = {}
        for K in (1, 4):
            ms = []
            vk.knn(q_np, t_np, K)
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                vk.knn(q_np, t_np, K)
                ms.append(1e3 * (time.perf_counter() - t0))
            case['numpy_ms'][str(K)] = _stats(ms)
        model.grid(d_t)                                                  # (vk.knn used its own cached handle; kept explicit)
        if cKDTree is not None:
            case['ckdtree_ms'] = {}
            q64, t64 = q_np.astype(np.float64), t_np.astype(np.float64)
            for K in a.K:
                ms = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    cKDTree(t64).query(q64, K, workers=16)
                    ms.append(1e3 * (time.perf_counter() - t0))
                case['ckdtree_ms'][str(K)] = _stats(ms)
        res['cases'].append(case)
    res['scipy'] = cKDTree is not None
    res['device'] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
