"""The tracked box stage with the moving tracks' points measured on the host and on the GPU (device.moving_boxes), one JSON line (also
written to profiles/moving_boxes_bench.json):

    python tools/bench_moving_boxes.py [--frames 199] [--points 150000] [--warmup 10] [--rounds 5] [--reps 50] [--out profiles/moving_boxes_bench.json]

Workload: the command line's synthetic sequence (tools/time_cli.py's: 199 frames of 150 000 points, default 9-stage list).  When the
run reaches the box stage, ZeroShotDetector._fit_boxes_tracked is repeated on the very same tracker and frame states, in both modes in
turn, with the detector's part timers on:
  host / device   wall ms of one _fit_boxes_tracked and of its `boxes.*` parts (whole sequence; `per_frame_ms` divides the total by the
                  frames): `warmup` runs of each mode, then `rounds` rounds of (host, device); median with min and max
  kernel          vg_cluster_oriented_extents alone on the pairs of the frame that has the most, inputs on the GPU, between two HIP
                  events: `warmup` launches, then `rounds` measurements of `reps` launches, ms per launch
`equal`: both modes left the same boxes, static_track flags and valid flags in every frame.
"""
import argparse
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _stats(v):
    return {'median': round(float(np.median(v)), 4), 'min': round(float(min(v)), 4), 'max': round(float(max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=199)
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moving_boxes_bench.json'))
    a = ap.parse_args()
    import preprocess_data
    from vilgod_amd import zero_shot_detector as zsd
    res = {'metric': 'moving_boxes_stage_ms', 'frames': a.frames, 'points': a.points, 'warmup': a.warmup, 'rounds': a.rounds, 'reps': a.reps}
    fit = zsd.ZeroShotDetector._fit_boxes_tracked

    def once(det, mode, valid_only, method):
        det.moving_boxes, det._detail_on, det.detail_ms = mode, True, {}
        for fs in det.lidar_frame_list:
            fs.boxes = None
        t0 = time.perf_counter()
        fit(det, valid_only, method)
        wall = 1e3 * (time.perf_counter() - t0)
        state = [(fs.boxes, fs.static_track.copy(), fs.valid.copy()) for fs in det.lidar_frame_list]
        return wall, {k: v for k, v in det.detail_ms.items() if k.startswith('boxes.')}, state

    def measured(det, valid_only, method=None):
        keep = det.moving_boxes, det._detail_on, det.detail_ms
        pairs = []
        extents = det._moving_extents
        det._moving_extents = lambda p: (pairs.clear(), pairs.extend(p), extents(p))[2]
        runs = {'host': [], 'device': []}
        for mode in runs:
            for _ in range(a.warmup):
                once(det, mode, valid_only, method)
        for _ in range(a.rounds):
            for mode in runs:
                runs[mode].append(once(det, mode, valid_only, method))
        for mode, rr in runs.items():
            parts = sorted({k for _, d, _ in rr for k in d})
            res[mode] = {'wall_ms': _stats([w for w, _, _ in rr]), 'per_frame_ms': round(float(np.median([w for w, _, _ in rr])) / a.frames, 4),
                         'parts_ms': {k: _stats([d.get(k, 0.0) for _, d, _ in rr]) for k in parts}}
        sh, sd = runs['host'][-1][2], runs['device'][-1][2]
        res['equal'] = all((b0 is None) == (b1 is None) and (b0 is None or np.array_equal(b0, b1, equal_nan=True)) and np.array_equal(s0, s1)
                           and np.array_equal(v0, v1) for (b0, s0, v0), (b1, s1, v1) in zip(sh, sd))
        moving = [t for t in det.tracker.tracks_valid if not t.static]
        res['tracks'] = {'valid': len(det.tracker.tracks_valid), 'moving': len(moving), 'moving_entries': len(pairs)}
        # ---- the kernel alone, on the frame with the most pairs ----
        by_frame = {}
        for p in pairs:
            by_frame.setdefault(p[2][0], []).append(p)
        if by_frame:
            fnr, pp = max(by_frame.items(), key=lambda kv: len(kv[1]))
            fs, dev = det.lidar_frame_list[fnr], det.pipe.device
            rows = sorted({p[2][1] for p in pp})
            X = det._ref_and_nonground(fnr)[1]
            d_index, d_seg = det._cluster_lists(fnr, rows)
            d_pc = torch.tensor([rows.index(p[2][1]) for p in pp], dtype=torch.int32, device=dev)
            d_c3 = torch.from_numpy(np.array([p[4] for p in pp], dtype=np.float32)).to(dev)
            d_rot = torch.from_numpy(np.array([p[3] for p in pp], dtype=np.float64)).to(dev)
            d_out = torch.empty((len(pp), 6), dtype=torch.float64, device=dev)
            call = lambda: det.pipe.oriented_extents(X, d_index, d_seg, d_pc, d_c3, d_rot, out=d_out)
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.reps)
            n = [int(fs.seg_off[r + 1] - fs.seg_off[r]) for r in rows]
            res['kernel'] = {'frame': int(fnr), 'pairs': len(pp), 'clusters': len(rows), 'points': int(sum(n)), 'largest_cluster': int(max(n)),
                             'ms_per_launch': _stats(ms)}
        det._moving_extents = extents
        det.moving_boxes, det._detail_on, det.detail_ms = keep
        for fs in det.lidar_frame_list:
            fs.boxes = None
        fit(det, valid_only, method)                          # the run goes on from the configured mode's result

    zsd.ZeroShotDetector._fit_boxes_tracked = measured
    with tempfile.TemporaryDirectory() as root:
        logging.disable(logging.INFO)
        preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', f'dataset.SYNTHETIC.frames_per_sequence={a.frames}',
                              f'dataset.SYNTHETIC.points_per_frame={a.points}', 'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0',
                              f'device.max_points={2 * a.points}', 'device.overlap_sequences=False', 'paths.clip_model=/nonexistent'])
    zsd.ZeroShotDetector._fit_boxes_tracked = fit
    res['gpu'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
