"""Points in boxes on the benchmark's frame, the GPU kernel beside the host entry point and `label_proposals` end to end, one JSON
line (also written to profiles/points_in_boxes_bench.json):

    python tools/bench_points_in_boxes.py [--points 150000] [--boxes 64 256 1024] [--reps 50] [--rounds 5] [--out profiles/points_in_boxes_bench.json]

Workload: the first frame of bench.py (synthetic.make_frame(1, 150 000 points, 60 objects)) against 64, 256 and 1024 seeded boxes
(1.5 .. 5 m, any heading, centred on points of the frame), float32 as pointcloud_utils.points_in_boxes passes them.
  device_gpu     vg_points_in_boxes on points and boxes already on the GPU, between two HIP events: ms per launch
  device         the same launches, wall time with the stream drained at the end
  host           points_in_boxes_host (vg_points_in_boxes_host, one CPU thread) on the same arrays: one pass per round
  label_proposals   PseudoLabelPipeline.label_proposals on the frame's 60 annotation boxes, numpy in, result dict out (upload, to_ref,
                 the kernel, packing, render + ViT + scores, vote), with the seeded ViT-B/16 weights bench.py runs on
10 warm-up launches, then the median of `rounds` measurements of `reps` launches with their min and max.  `inside`: the share of the
points inside some box; `equal_host`: the kernel's indices equal the host entry point's.
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


def seeded_boxes(points, m, seed=0):
    rng = np.random.default_rng(seed)
    at = points[rng.integers(0, len(points), m), :3].astype(np.float64)
    return np.c_[at + rng.normal(0, 0.2, (m, 3)), rng.uniform(1.5, 5.0, (m, 2)), rng.uniform(1.0, 3.0, m),
                 rng.uniform(-np.pi, np.pi, m)].astype(np.float32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--boxes', type=int, nargs='*', default=[64, 256, 1024])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-pipeline', action='store_true', help='skip the label_proposals measurement')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'points_in_boxes_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import points_in_boxes as pib, synthetic
    dev = torch.device('cuda:0')
    pts, meta = synthetic.make_frame(1, a.points, n_objects=a.objects, return_meta=True)
    d_pts = torch.from_numpy(pts).to(dev).unsqueeze(0)
    res = {'metric': 'points_in_boxes_ms', 'points': a.points, 'reps': a.reps, 'rounds': a.rounds, 'cases': []}
    for m in a.boxes:
        boxes = seeded_boxes(pts, m)
        d_boxes = torch.from_numpy(boxes).to(dev).unsqueeze(0)
        got = pib.points_in_boxes_gpu(d_pts, d_boxes)[0].cpu().numpy()
        host_ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            want = pib.points_in_boxes_host(pts, boxes)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        call = lambda: pib.points_in_boxes_gpu(d_pts, d_boxes)
        res['cases'].append({'boxes': m, 'inside': round(float(np.mean(want >= 0)), 4), 'equal_host': bool(np.array_equal(got, want)),
                             'device_gpu_ms': _measure(call, a.reps, a.rounds, events=True),
                             'device_ms': _measure(call, a.reps, a.rounds), 'host_ms': _stats(host_ms)})
    if not a.no_pipeline:
        from vilgod_amd.pipeline import PseudoLabelPipeline
        pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent')      # (bench.py's weights)
        poses = synthetic.make_poses(2)
        props = np.array([[*o['center'], o['dims'][0] + 0.3, o['dims'][1] + 0.3, o['dims'][2] + 0.3, o['yaw']] for o in meta['objects']])
        fs, out = pipe.label_proposals(pts, poses[1], poses[0], props)
        res['label_proposals'] = {'proposals': len(props), 'detections': int(fs.n_detections), 'labelled': int(len(out['name'])),
                                  'weights': pipe.clip.weights_source,
                                  'ms': _measure(lambda: pipe.label_proposals(pts, poses[1], poses[0], props), max(1, a.reps // 10), a.rounds, warmup=3)}
    res['device'] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
