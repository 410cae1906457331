"""GPU time of fit_bounding_boxes_simple's box fits per bench-shaped frame (150k synthetic points, bench.py's 60 objects: ~86
clusters), one JSON line:

    python tools/bench_box_methods.py [--frames 4] [--reps 20]

  minimum_bounding_rectangle  vg_cluster_boxes (box_mode='fast'); the default box_mode='reference' runs qhull on the host instead,
                              its wall time per frame (in this thread) is reported beside it
  closeness_rectangle         vg_cluster_lshape, 46 angles (delta 2)
  variance_rectangle          vg_cluster_lshape, 901 angles (delta 0.1)
GPU times are HIP event pairs around `reps` back-to-back launches over all of a frame's clusters, averaged over the frames.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    from vilgod_amd import synthetic, boxes as vb
    from vilgod_amd.frame_state import pack_clusters
    from vilgod_amd.pipeline import PseudoLabelPipeline
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 16, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    poses = synthetic.make_poses(2)
    fits = {
        'minimum_bounding_rectangle': lambda X, di, ds: pipe.boxes(X, di, ds),
        'closeness_rectangle': lambda X, di, ds: pipe.lshape_boxes(X, di, ds, 'closeness_rectangle'),
        'variance_rectangle': lambda X, di, ds: pipe.lshape_boxes(X, di, ds, 'variance_rectangle'),
    }
    ms = {k: [] for k in fits}
    host_ms, n_clusters, n_points = [], [], []
    for f in range(a.frames):
        pts = synthetic.make_frame(1 + f, a.points, n_objects=a.objects)
        fs, d_ref, d_X, gidx = pipe.prepare(pts, poses[1], poses[0])
        labels, probs = pipe.cluster(d_X)
        _, index, seg = pack_clusters(labels, probs, pipe.prob_threshold)
        d_index = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
        d_seg = torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
        n_clusters.append(len(seg) - 1)
        n_points.append(int(seg[-1]))
        for name, fn in fits.items():
            for _ in range(3):
                fn(d_X, d_index, d_seg)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn(d_X, d_index, d_seg)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.reps)
        xy = d_X[:, :2].cpu().numpy()
        zmin, zmax = pipe.z_extent(d_X, d_index, d_seg)
        t0 = time.perf_counter()
        vb.reference_boxes(xy, index, seg, zmin, zmax)
        host_ms.append(1000 * (time.perf_counter() - t0))
    out = {'metric': 'box_fit_ms_per_frame', 'frames': a.frames, 'points_per_frame': a.points,
           'clusters_per_frame': float(np.mean(n_clusters)), 'clustered_points_per_frame': float(np.mean(n_points)),
           'gpu_ms': {k: round(float(np.mean(v)), 4) for k, v in ms.items()},
           'minimum_bounding_rectangle_reference_mode_host_ms': round(float(np.mean(host_ms)), 3),
           'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
