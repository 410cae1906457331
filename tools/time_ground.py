"""Ground pass alone, one JSON line:

    python tools/time_ground.py [--rounds 5] [--reps 50] [--json FILE]

Frame sets, each a sequence on one handle (the adaptive state carries over, as in a run):
    synthetic_150k   four synthetic benchmark frames of 150 000 points
    kitti_fixture    the KITTI scans under tests/golden/ (left out when there are none)
10 warm-up passes over the set (they also fill the threshold stores), then the median of `rounds` measurements with their min and max.
A measurement is `reps` back-to-back passes over the set, ending in a synchronise: wall time per ground pass, launches included.
Set VILGOD_HIP_LIB to time another build of the library.
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


def measure(pipe, frames, reps, rounds, warmup=10):
    pipe.new_sequence()
    for _ in range(warmup):
        for f in frames:
            pipe.ground(f)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            for f in frames:
                pipe.ground(f)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / (reps * len(frames)))
    return {'median': round(float(np.median(out)), 4), 'min': round(min(out), 4), 'max': round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--json', default=None, help='also write the line to this file')
    a = ap.parse_args()
    from vilgod_amd import _lib, synthetic
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pipe = PseudoLabelPipeline(device='cuda:0', max_points=200_000, clip_model_path='/nonexistent', box_workers=0)
    sets = {'synthetic_150k': [pipe.upload(synthetic.make_frame(1 + i, 150_000, n_objects=60)) for i in range(4)]}
    golden = os.path.join(ROOT, 'tests', 'golden')
    scans = sorted(f for f in os.listdir(golden) if f.startswith('kitti_') and f.endswith('.bin'))
    if scans:
        sets['kitti_fixture'] = [pipe.upload(np.fromfile(os.path.join(golden, f), dtype=np.float32).reshape(-1, 4)) for f in scans]
    res = {'metric': 'ground_ms_per_pass', 'sets': {}}
    for name, frames in sets.items():
        res['sets'][name] = dict(measure(pipe, frames, a.reps, a.rounds), frames=len(frames), points=[int(f.shape[0]) for f in frames])
    res.update({'reps': a.reps, 'rounds': a.rounds, 'warmup_passes': 10, 'library': os.path.basename(_lib.LIB_PATH),
                'device': torch.cuda.get_device_name(0)})
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
