"""Ball query on the benchmark's frame: vg_cluster_ball_query beside vg_cluster_ball_count with the same arguments, one JSON line (also
written to --json, default profiles/ball_query_bench.json):

    python tools/bench_ball_query.py [--points 150000] [--reps 20] [--rounds 5] [--json profiles/ball_query_bench.json]

Workload: the non-ground points of bench.py's first frame (tools/bench_knn.py `nonground`: about 79 k points stay), queried against
themselves (`self`: count_neighbors_inter_frame's shape, and count_neighbors' seek column) and against the next frame's non-ground
points (`next`: count_neighbors' other columns).  The queries are in `entropy.spatial_order`; the grid is built once per target set,
outside the timing.  Settings (radius, nsample): (0.3, 1000) count_neighbors, (0.2, 100) the two-frame clusterer's
count_neighbors_inter_frame, (sqrt(0.1), 4) the moving-point test, (0.3, 16) a short table at the entropy radius.
  ball_query_gpu_ms   vg_cluster_ball_query into preallocated idx [nq, nsample] / cnt [nq], between two HIP events: ms per launch
  ball_count_gpu_ms   vg_cluster_ball_count(cap = nsample) with the same queries, grid and r2, in the same run
  cnt                 mean / max of cnt and the share of queries the cap cuts (cnt == nsample); cnt == the count is asserted
10 warm-up launches, then the median of `rounds` measurements of `reps` launches with their min and max.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_knn import _measure, nonground      # noqa: E402

SETTINGS = ((0.3, 1000), (0.2, 100), (math.sqrt(0.1), 4), (0.3, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=os.path.join(ROOT, 'profiles', 'ball_query_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import synthetic
    from vilgod_amd.cluster_handle import GridQueries
    from vilgod_amd.entropy import spatial_order
    from vilgod_amd.pipeline import PseudoLabelPipeline
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent')
    poses = synthetic.make_poses(2)
    frames = [nonground(pipe, synthetic, s, a.points, a.objects, poses) for s in (1, 2)]
    del pipe
    model = GridQueries(max(len(f) for f in frames), dev)
    res = {'metric': 'ball_query_ms', 'points': a.points, 'nonground': [len(f) for f in frames], 'reps': a.reps, 'rounds': a.rounds, 'cases': []}
    d_q = torch.from_numpy(frames[0]).to(dev)
    d_q = d_q.index_select(0, spatial_order(d_q)).contiguous()
    nq = d_q.shape[0]
    for name, t_np in (('self', frames[0]), ('next', frames[1])):
        model.grid(torch.from_numpy(t_np).to(dev))
        case = {'targets': name, 'n_query': nq, 'n_target': len(t_np), 'settings': []}
        for radius, nsample in SETTINGS:
            r2 = np.float32(radius) * np.float32(radius)
            out = (torch.empty((nq, nsample), dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
            counts = torch.empty(nq, dtype=torch.int32, device=dev)
            query = lambda: model.ball_query(d_q, r2, nsample, out=out)
            count = lambda: model.ball_count(d_q, r2, nsample, out=counts)
            s = {'radius': round(radius, 6), 'r2': float(r2), 'nsample': nsample, 'idx_mb': round(4e-6 * nq * nsample, 1),
                 'ball_query_gpu_ms': _measure(query, a.reps, a.rounds, events=True),
                 'ball_count_gpu_ms': _measure(count, a.reps, a.rounds, events=True)}
            assert torch.equal(out[1], counts)
            c = out[1].float()
            s['cnt'] = {'mean': round(float(c.mean()), 2), 'max': int(c.max()), 'capped': round(float((out[1] == nsample).float().mean()), 4)}
            case['settings'].append(s)
            del out
        res['cases'].append(case)
    res['device'] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
