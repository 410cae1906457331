"""Rotated-box IoU of one sequence's evaluation, host numpy against the GPU kernel, one JSON line (also written to
profiles/iou_bench.json):

    python tools/bench_iou.py [--groups 199] [--dets 90] [--gts 100] [--reps 20] [--rounds 5] [--out profiles/iou_bench.json]

Workload: `groups` independent matrices of `dets` x `gts` seeded boxes -- a 199-frame sequence with ~90 detections against ~100
ground truths per frame, ~1.8 M pairs; every detection is drawn around a ground truth, the rest of its row is far away, as in a frame.
  host          the loop detection_metrics runs: evaluation.iou3d_matrix once per group (wall time of one pass, median of `rounds`)
  device        iou.iou_groups on boxes already on the GPU: offsets H2D, vg_boxes_iou3d (one read-back of the offsets, ONE launch), stream
                drained -- wall time per call over `reps` back-to-back calls
  device_gpu    the same calls between two HIP events
  device_e2e    evaluation.iou3d_matrices_device: numpy in, numpy out (boxes H2D, the launch, the result D2H, the per-group views)
10 warm-up runs, then the median of `rounds` measurements with their min and max.  max_abs_diff: device against host over all pairs.
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


def workload(groups, dets, gts, seed=0):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(groups):
        g = np.c_[rng.uniform(-75, 75, (gts, 2)), rng.uniform(-1, 1, gts), rng.uniform(3.5, 5.5, gts), rng.uniform(1.6, 2.4, gts),
                  rng.uniform(1.4, 2.0, gts), rng.uniform(-np.pi, np.pi, gts)]
        src = rng.integers(0, gts, dets)
        d = g[src] + np.c_[rng.normal(0, 0.5, (dets, 2)), rng.normal(0, 0.1, dets), rng.normal(0, 0.2, (dets, 3)), rng.normal(0, 0.15, dets)]
        pairs.append((d, g))
    return pairs


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
    return {'median': round(float(np.median(out)), 4), 'min': round(float(min(out)), 4), 'max': round(float(max(out)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=199)
    ap.add_argument('--dets', type=int, default=90)
    ap.add_argument('--gts', type=int, default=100)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'iou_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import evaluation as ev, iou
    dev = torch.device('cuda:0')
    pairs = workload(a.groups, a.dets, a.gts)

    def host_pass():
        return [ev.iou3d_matrix(d, g) for d, g in pairs]

    host_ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        want = host_pass()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    a_off = np.cumsum([0] + [len(d) for d, _ in pairs])
    b_off = np.cumsum([0] + [len(g) for _, g in pairs])
    d_a = torch.from_numpy(np.concatenate([d for d, _ in pairs])).to(dev)
    d_b = torch.from_numpy(np.concatenate([g for _, g in pairs])).to(dev)

    def device_call():
        return iou.iou_groups(d_a, a_off, d_b, b_off)

    got = ev.iou3d_matrices_device(pairs)
    diff = max(float(np.abs(x - y).max()) for x, y in zip(got, want))
    res = {'metric': 'boxes_iou3d_ms_per_sequence', 'groups': a.groups, 'dets': a.dets, 'gts': a.gts,
           'pairs': int(sum(len(d) * len(g) for d, g in pairs)), 'intersecting_pairs': int(sum(np.count_nonzero(w) for w in want)),
           'host_ms': {'median': round(float(np.median(host_ms)), 2), 'min': round(min(host_ms), 2), 'max': round(max(host_ms), 2)},
           'device_ms': _measure(device_call, a.reps, a.rounds),
           'device_gpu_ms': _measure(device_call, a.reps, a.rounds, events=True),
           'device_e2e_ms': _measure(lambda: ev.iou3d_matrices_device(pairs), max(1, a.reps // 4), a.rounds, warmup=3),
           'max_abs_diff': diff, 'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
