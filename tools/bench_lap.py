"""Linear assignment, the GPU kernel beside the scipy loop the evaluation runs today (one JSON line with --json, also written to
profiles/lap_bench.json):

    python tools/bench_lap.py [--json] [--reps 5] [--rounds 5] [--no-metrics] [--out profiles/lap_bench.json]

Workloads: seeded IoU-like weights (per row about three entries drawn from 0.3 .. 1, the rest 0, as a thresholded IoU matrix looks),
costs -w with "stay unassigned" at 0, which is what detection_metrics hands the solver:
    one_64, one_256, one_1024   one group of 64 x 64, 256 x 256, 1024 x 1024, one snapshot after the last row
    600_x_30                    600 groups of 24 .. 36 rows and columns, rows in a seeded order, a snapshot after EVERY prefix
  scipy         scipy.optimize.linear_sum_assignment(-w[kept rows]) per group and prefix, as evaluation.detection_metrics calls it, one
                CPU thread: wall time, median of `rounds`
  host          lap.lap_groups_host (vg_lap_groups_host, one CPU thread): wall time of one call, median of `rounds`
  device        lap.lap_groups on costs and an order already on the GPU (the call uploads its small offset tables and fills its outputs
                from torch's caching allocator; one launch), stream drained -- wall time per call over `reps` back-to-back calls
  device_gpu    the same calls between two HIP events
10 warm-up calls, then the median of `rounds` measurements with their min and max.  `equal`: the device's snapshots and statuses are
the host form's; `same_pairs`: the pairs of positive weight are scipy's in every snapshot.
`metrics`: one whole evaluation.detection_metrics call on a seeded 199-frame scene set (types 1, 2, 4; up to 40 predictions and 40
ground truths per frame and type) in the four (iou, match) modes: wall time, one warm-up call on a 3-frame set, then the median of 3.
No speed-up is assumed: one group is one wave's serial chain, and the numbers say where that loses.
Not measured here: a captured graph's replay, a detector's real output, more than one GPU, the tracker's matcher (not served).
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


def weights(n, m, seed):
    rng = np.random.default_rng([4100, seed, n, m])
    hit = rng.uniform(size=(n, m)) < 3.0 / max(m, 3)
    return np.where(hit, rng.uniform(0.3, 1.0, (n, m)), 0.0)


def workload(name):
    if name.startswith('one_'):
        n = int(name.split('_')[1])
        mats = [weights(n, n, 0)]
        orders = [np.arange(n, dtype=np.int32)]
        prefixes = [[n]]
    else:
        rng = np.random.default_rng(4200)
        mats = [weights(int(rng.integers(24, 37)), int(rng.integers(24, 37)), 1 + g) for g in range(600)]
        orders = [rng.permutation(w.shape[0]).astype(np.int32) for w in mats]
        prefixes = [list(range(1, w.shape[0] + 1)) for w in mats]
    sizes = np.array([w.size for w in mats])
    return {'w': mats, 'orders': orders, 'prefixes': prefixes, 'cost': -np.concatenate([w.reshape(-1) for w in mats]),
            'cost_off': np.cumsum(sizes) - sizes, 'row_off': np.cumsum([0] + [w.shape[0] for w in mats]),
            'col_off': np.cumsum([0] + [w.shape[1] for w in mats])}


def scipy_loop(wl):
    from scipy.optimize import linear_sum_assignment
    out = []
    for w, order, prefixes in zip(wl['w'], wl['orders'], wl['prefixes']):
        for k in prefixes:
            keep = np.sort(order[:k])
            rr, cc = linear_sum_assignment(-w[keep])
            good = w[keep][rr, cc] > 0
            out.append(set(zip(keep[rr[good]].tolist(), cc[good].tolist())))
    return out


def pairs_of(wl, match, match_off):
    out, s = [], 0
    for w, prefixes in zip(wl['w'], wl['prefixes']):
        for _ in prefixes:
            col = match[match_off[s]:match_off[s] + w.shape[0]]
            rows = np.flatnonzero(col >= 0)
            out.append({(int(i), int(col[i])) for i in rows if w[i, col[i]] > 0})
            s += 1
    return out


def _stats(out, digits=4):
    return {'median': round(float(np.median(out)), digits), 'min': round(float(min(out)), digits), 'max': round(float(max(out)), digits)}


def _wall(fn, rounds):
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        res = fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return _stats(out, 3), res


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


def scene_set(frames, seed=0, most=40):
    """the positional arguments of detection_metrics but the config: `frames` frames, types 1, 2 and 4, predictions scattered on ground truth"""
    rng = np.random.default_rng(4300 + seed)
    pf, pb, pt, ps, gf, gb, gt, gl = [], [], [], [], [], [], [], []
    for f in range(frames):
        for t in (1, 2, 4):
            ng, n_p = int(rng.integers(1, most + 1)), int(rng.integers(1, most + 1))
            size = {1: (4.5, 2.0, 1.6), 2: (0.8, 0.7, 1.7), 4: (1.8, 0.7, 1.6)}[t]
            g = np.c_[rng.uniform(-60, 60, (ng, 2)), rng.uniform(-1, 1, ng), size * rng.uniform(0.8, 1.2, (ng, 3)), rng.uniform(-np.pi, np.pi, ng)]
            p = g[rng.integers(0, ng, n_p)] + np.c_[rng.normal(0, 0.25, (n_p, 2)) * size[0] / 2, rng.normal(0, 0.1, n_p),
                                                    rng.normal(0, 0.1, (n_p, 3)), rng.normal(0, 0.2, n_p)]
            pf += [f] * n_p; pb.append(p); pt += [t] * n_p; ps += list(np.round(rng.uniform(0.05, 0.99, n_p), 3))
            gf += [f] * ng; gb.append(g); gt += [t] * ng; gl += list(rng.integers(1, 3, ng))
    return (np.array(pf, np.int64), np.concatenate(pb).reshape(-1, 7), np.array(pt, np.int64), np.array(ps, np.float64),
            np.array(gf, np.int64), np.concatenate(gb).reshape(-1, 7), np.array(gt, np.int64), np.array(gl, np.int8))


def bench_metrics(rounds=3):
    from vilgod_amd import evaluation as ev
    cfg = ev.build_config(difficulties=[1, 2], breakdown_range=True, iou_thresholds=(0.5, 0.3, 0.4, 0.35))
    small, full = scene_set(3, 1) + (cfg,), scene_set(199) + (cfg,)
    res = {'frames': 199, 'predictions': int(len(full[0])), 'ground_truths': int(len(full[4])), 'modes': {}}
    base = None
    for iou in ('host', 'device'):
        for match in ('host', 'device'):
            ev.detection_metrics(*small, iou=iou, match=match)
            ms, out = _wall(lambda: ev.detection_metrics(*full, iou=iou, match=match), rounds)
            base = out if base is None else base
            res['modes'][f'iou_{iou}_match_{match}'] = {'ms': ms, 'max_abs_diff_to_host_host': float(max(abs(out[k][0] - base[k][0]) for k in base))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', action='store_true', help='print the one JSON line only')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-metrics', action='store_true', help='leave out the whole-evaluation timings')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lap_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import lap
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    res = {'metric': 'lap_groups_ms_per_call', 'unassigned_cost': 0.0, 'cases': {}}
    for name in ('one_64', 'one_256', 'one_1024', '600_x_30'):
        wl = workload(name)
        order = np.concatenate(wl['orders'])
        scipy_ms, want_pairs = _wall(lambda: scipy_loop(wl), a.rounds)
        host_ms, want = _wall(lambda: lap.lap_groups_host(wl['cost'], wl['cost_off'], wl['row_off'], wl['col_off'], 0.0, order, wl['prefixes']),
                              a.rounds)
        d_cost, d_order = torch.from_numpy(wl['cost']).to(dev), torch.from_numpy(order).to(dev)

        def device_call():
            return lap.lap_groups(d_cost, wl['cost_off'], wl['row_off'], wl['col_off'], 0.0, d_order, wl['prefixes'])

        got = device_call()
        equal = bool(got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[3].cpu().numpy().tobytes() == want[3].tobytes())
        res['cases'][name] = {'groups': len(wl['w']), 'snapshots': int(len(want[1])), 'equal': equal,
                              'same_pairs': pairs_of(wl, want[0], want[1]) == want_pairs, 'scipy_ms': scipy_ms, 'host_ms': host_ms,
                              'device_ms': _measure(device_call, a.reps, a.rounds), 'device_gpu_ms': _measure(device_call, a.reps, a.rounds, events=True)}
        if not a.json:
            print(name, json.dumps(res['cases'][name]), flush=True)
    if not a.no_metrics:
        res['metrics'] = bench_metrics()
    res.update({'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
