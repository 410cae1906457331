"""Rotated-box NMS, the GPU kernels beside the host entry point, one JSON line (also written to profiles/nms_bench.json):

    python tools/bench_nms.py [--thresh 0.5] [--reps 20] [--rounds 5] [--out profiles/nms_bench.json]

Workloads: seeded crowded groups (boxes of 0.5 .. 6 m x 0.5 .. 3 m at any heading in 16 m x 16 m, as tests/iou_ref.crowd draws them:
most pairs of a group intersect), float32 boxes and scores, mode 'rotated':
    one_512      one group of 512 rows
    one_4096     one group of 4096 rows (the cap)
    199_x_100    199 groups of 100 rows in one call (a sequence's frames)
  host          nms.nms_groups_host (vg_boxes_nms_host, one CPU thread): wall time of one call, median of `rounds`
  device        nms.nms_groups on tensors and an offset table already on the GPU (the output fills, the work buffer from torch's caching
                allocator, three launches), stream drained -- wall time per call over `reps` back-to-back calls
  device_gpu    the same calls between two HIP events
10 warm-up calls, then the median of `rounds` measurements with their min and max.  `equal`: the device's keep lists and counts are
the host's.  Not measured here: a captured graph's replay, a detector's real output.
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


def crowd(n, seed):
    rng = np.random.default_rng(900 + seed)
    return np.c_[20 + rng.uniform(-8, 8, n), -30 + rng.uniform(-8, 8, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 6, n), rng.uniform(0.5, 3, n),
                 rng.uniform(1, 3, n), rng.uniform(-4, 4, n)].astype(np.float32)


def workload(groups, size, seed=0):
    boxes = np.concatenate([crowd(size, 1000 * seed + g) for g in range(groups)])
    scores = np.random.default_rng(77 + seed).uniform(0.05, 0.99, len(boxes)).astype(np.float32)
    return boxes, scores, size * np.arange(groups + 1)


def _stats(out, digits=4):
    return {'median': round(float(np.median(out)), digits), 'min': round(float(min(out)), digits), 'max': round(float(max(out)), digits)}


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
    ap.add_argument('--thresh', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nms_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import nms
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    res = {'metric': 'boxes_nms_ms_per_call', 'mode': 'rotated', 'thresh': a.thresh, 'dtype': 'float32', 'cases': {}}
    for name, groups, size in (('one_512', 1, 512), ('one_4096', 1, 4096), ('199_x_100', 199, 100)):
        boxes, scores, off = workload(groups, size)
        host_ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            want = nms.nms_groups_host(boxes, scores, off, a.thresh)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        d_boxes, d_scores = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
        d_off = torch.from_numpy(off.astype(np.int32)).to(dev)

        def device_call():
            return nms.nms_groups(d_boxes, d_scores, d_off, a.thresh, max_group=size)

        keep, counts = device_call()
        equal = bool(np.array_equal(keep.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1]))
        res['cases'][name] = {'groups': groups, 'rows_per_group': size, 'kept': int(want[1].sum()), 'equal': equal,
                              'host_ms': _stats(host_ms, 3), 'device_ms': _measure(device_call, a.reps, a.rounds),
                              'device_gpu_ms': _measure(device_call, a.reps, a.rounds, events=True)}
    res.update({'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
