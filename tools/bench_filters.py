"""GPU time of the cluster filters per bench-shaped frame (150k synthetic points, bench.py's 60 objects: ~86 clusters), one JSON line:

    python tools/bench_filters.py [--frames 4] [--reps 50] [--rounds 5]

  shipped_three   filter_by_number_points, filter_by_height, filter_by_plane_distance through vg_cluster_filter (the default path)
  all_seven       those plus aspect ratio, volume, area and ephemeral score (waymo.yaml's thresholds) through vg_cluster_filter_ex,
                  with seeded per-point scores
GPU times are HIP event pairs around `reps` back-to-back launches over all of a frame's clusters, after 10 warm-up launches; the
median of `rounds` such measurements per frame, averaged over the frames (min / max of the rounds are reported beside it).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    from vilgod_amd import synthetic
    from vilgod_amd._lib import lib, ptr, stream_ptr, check, FILTER_NAMES, FILTER_NSTATS
    from vilgod_amd.frame_state import pack_clusters
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 16, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    cfg = default_preprocessor_cfg()['clustering']
    cfg['filters'] = cfg['filters'] + [
        dict(name='filter_by_aspect_ratio', args=dict(logic='and', min_aspect_ratio=1.0, max_aspect_ratio=5.0)),
        dict(name='filter_by_volume', args=dict(logic='and', min_volume=0.5)),
        dict(name='filter_by_area', args=dict(logic='and', min_area=0.35)),
        dict(name='filter_by_ephemeral_score', args=dict(logic='or', percentile=20, min_percentile_pp_score=0.7))]
    cfg['filters_active'] = [f['name'] for f in cfg['filters']]
    P = PseudoLabelPipeline._parse_filters(cfg)['params']
    poses = synthetic.make_poses(2)
    ms = {'shipped_three': [], 'all_seven': []}
    spread = {'shipped_three': [], 'all_seven': []}
    n_clusters, n_points, n_max = [], [], []
    for f in range(a.frames):
        pts = synthetic.make_frame(1 + f, a.points, n_objects=a.objects)
        fs, d_ref, d_X, gidx = pipe.prepare(pts, poses[1], poses[0])
        labels, probs = pipe.cluster(d_X)
        _, index, seg = pack_clusters(labels, probs, pipe.prob_threshold)
        d_index = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
        d_seg = torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
        C = len(seg) - 1
        n_clusters.append(C)
        n_points.append(int(seg[-1]))
        n_max.append(int(np.diff(seg).max()))
        d_plane = torch.from_numpy(pipe.ground_plane(d_ref, gidx)).to(dev)
        d_scores = torch.from_numpy(np.random.default_rng(f).uniform(0, 1, d_X.shape[0]).astype(np.float32)).to(dev)
        stats6 = torch.empty((C, 6), dtype=torch.float32, device=dev)
        stats = torch.empty((C, FILTER_NSTATS), dtype=torch.float64, device=dev)
        verdict = torch.empty((C, len(FILTER_NAMES)), dtype=torch.uint8, device=dev)
        valid = torch.empty(C, dtype=torch.uint8, device=dev)
        runs = {
            'shipped_three': lambda: check(lib.vg_cluster_filter(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, ptr(d_plane), 10, 999999,
                                                                 1.0, 0.5, 0.3, 6.0, ptr(stats6), ptr(valid), stream_ptr()), 'vg_cluster_filter'),
            'all_seven': lambda: check(lib.vg_cluster_filter_ex(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, ptr(d_plane), ptr(d_scores),
                                                                ctypes.byref(P), ptr(stats), ptr(verdict), ptr(valid), stream_ptr()),
                                       'vg_cluster_filter_ex'),
        }
        for name, fn in runs.items():
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            rounds = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                rounds.append(e0.elapsed_time(e1) / a.reps)
            ms[name].append(float(np.median(rounds)))
            spread[name].append((min(rounds), max(rounds)))
    out = {'metric': 'cluster_filter_ms_per_frame', 'frames': a.frames, 'points_per_frame': a.points,
           'clusters_per_frame': float(np.mean(n_clusters)), 'clustered_points_per_frame': float(np.mean(n_points)),
           'largest_cluster_points': int(max(n_max)),
           'gpu_ms': {k: round(float(np.mean(v)), 4) for k, v in ms.items()},
           'gpu_ms_round_min_max': {k: [round(float(np.mean([s[0] for s in v])), 4), round(float(np.mean([s[1] for s in v])), 4)]
                                    for k, v in spread.items()},
           'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
