"""GPU time of the clustering model's GPU stage against min_samples (k) on the non-ground points of one synthetic 150k-point frame,
one JSON line:

    python tools/bench_min_samples.py [--k 15 16 24 32 48 64] [--reps 10] [--rounds 5] [--no-kernel-trace]

  mst_ms        the whole `HDBSCAN.mst()` call (grid, core distances, Boruvka rounds with their host reads, edge sort): host clock
                around `reps` back-to-back calls that end in a device synchronise, after 10 warm-up calls; median of `rounds` such
                measurements, with the rounds' min / max beside it
  core_ms       the core-distance stage alone = the kernel time of k_cl_blocks + the two cooperative phases (k_cl_core_blk,
                k_cl_core_far; k <= 15: register list / 16-lane list, k >= 16: LDS heap / wave-wide list) per call, from a
                kernel trace of the same call sequence in a process of its own per k (`rocprofv3 --kernel-trace`, this file as
                `--worker`); the same warm-up, median and min / max
  phase_b_share the share of queries phase A hands to phase B (read from the library's VG_CLUSTER_DEBUG line of one extra call)
`--k 15` alone uses nothing newer than min_samples <= 15, so the same file measures an older build for comparison.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 10
CORE_KERNELS = ('k_cl_blocks', 'k_cl_core_blk', 'k_cl_core_far')


def _model(k, n):
    from vilgod_amd.hdbscan import HDBSCAN
    return HDBSCAN(min_cluster_size=15, min_samples=k, cluster_selection_epsilon=0.15, max_points=n + 16)


def _calls(model, X, reps, rounds):
    """10 warm-up calls, then rounds x reps timed ones -> ms per call of every round"""
    for _ in range(WARMUP):
        model.mst(X)
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            model.mst(X)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return out


def worker(a):
    X = torch.from_numpy(np.load(a.points_file)).cuda()
    _calls(_model(a.k[0], X.shape[0]), X, a.reps, a.rounds)


def _summary(per_round):
    return {'median': round(float(np.median(per_round)), 4), 'min': round(float(min(per_round)), 4), 'max': round(float(max(per_round)), 4)}


def traced_core_ms(k, points_file, reps, rounds):
    tmp = tempfile.mkdtemp(prefix='min_samples_trace_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', tmp, '-o', 'ms', '--', sys.executable, os.path.abspath(__file__),
               '--worker', '--k', str(k), '--points-file', points_file, '--reps', str(reps), '--rounds', str(rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f'kernel trace for k={k} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        files = glob.glob(os.path.join(tmp, '**', 'ms_kernel_trace.csv'), recursive=True)
        if len(files) != 1:
            raise RuntimeError(f'kernel trace for k={k}: expected one ms_kernel_trace.csv, found {files}')
        per_kind = {name: [] for name in CORE_KERNELS}
        for row in csv.DictReader(open(files[0])):
            for name in CORE_KERNELS:
                if name in row['Kernel_Name']:
                    per_kind[name].append((int(row['Start_Timestamp']), int(row['End_Timestamp']) - int(row['Start_Timestamp'])))
        calls = WARMUP + reps * rounds
        per_call = np.zeros(calls)
        for name, rows in per_kind.items():
            if len(rows) != calls:
                raise RuntimeError(f'kernel trace for k={k}: {len(rows)} launches of {name}, {calls} calls')
            per_call += np.array([d for _, d in sorted(rows)]) * 1e-6
        per_round = per_call[WARMUP:].reshape(rounds, reps).mean(1)
        return _summary(per_round)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def phase_b_share(k, X):
    """one call on a handle created with VG_CLUSTER_DEBUG set: the library reports the work-list sizes of the two phases on stderr"""
    os.environ['VG_CLUSTER_DEBUG'] = '1'
    try:
        model = _model(k, X.shape[0])
    finally:
        del os.environ['VG_CLUSTER_DEBUG']
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as f:
        os.dup2(f.fileno(), 2)
        try:
            model.mst(X)
            torch.cuda.synchronize()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors='replace')
    m = re.search(r'core distances: n (\d+), k (\d+).*?(\d+) queries left to the far phase', text)
    if not m or int(m.group(2)) != k:
        raise RuntimeError(f'no core-distance debug line for k={k} in:\n{text[-1000:]}')
    return int(m.group(3)) / int(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, nargs='+', default=[15, 16, 24, 32, 48, 64])
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-kernel-trace', action='store_true', help='skip core_ms (no rocprofv3 child processes)')
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--points-file', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from vilgod_amd import synthetic
    from vilgod_amd.pipeline import PseudoLabelPipeline
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 16, clip_model_path='/nonexistent')
    pts = pipe.upload(synthetic.make_frame(1, a.points))
    mask = pipe.ground(pts)
    X = pipe.to_ref(pts, np.eye(4))[mask == 0][:, :3].contiguous()
    n = X.shape[0]
    del pipe
    tmp = tempfile.mkdtemp(prefix='min_samples_points_')
    points_file = os.path.join(tmp, 'points.npy')
    np.save(points_file, X.cpu().numpy())
    try:
        per_k = {}
        for k in a.k:
            model = _model(k, n)
            mst = _summary(_calls(model, X, a.reps, a.rounds))
            entry = {'mst_ms': mst, 'boruvka_rounds': int(model.n_rounds_), 'phase_b_share': round(phase_b_share(k, X), 5)}
            del model
            entry['core_ms'] = None if a.no_kernel_trace else traced_core_ms(k, points_file, a.reps, a.rounds)
            per_k[str(k)] = entry
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({'metric': 'hdbscan_gpu_stage_ms_by_min_samples', 'points_per_frame': a.points, 'clustered_points': n, 'k': per_k,
                      'warmup': WARMUP, 'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)}))


if __name__ == '__main__':
    main()
