"""Cluster packing and valid-cluster selection, host path against device path, on bench-shaped frames (150k synthetic points, bench.py's
60 objects: ~79k non-ground points, ~90 clusters), one JSON line:

    python tools/bench_pack.py [--frames 3] [--reps 50] [--rounds 5] [--latency-frames 6]

  pack.host      what pack='host' does between the hierarchy stage and the first kernel that reads the lists: labels + probabilities D2H,
                 vg_pack_clusters_host, index / seg H2D
  pack.device    vg_pack_clusters + the 12-byte counts read-back            (pack.device_gpu: the kernels alone, HIP events)
  select.host    verdict D2H, numpy concatenation of the valid clusters' segments, sub-lists H2D
  select.device  vg_pack_select, stream drained                            (select.device_gpu: the kernels alone, HIP events)
Both paths contain host work and waits, so the figures are WALL times of `reps` back-to-back repetitions on an otherwise idle GPU, each
repetition ending with the data where the next stage needs it; 10 warm-up repetitions, the median of `rounds` such measurements per
frame, averaged over the frames (min / max of the rounds beside it).
front_stage_ms: pipeline.process_frame(timing=True) marks of one 150k-point frame in both modes (a device synchronisation after every
mark: latency of a lone frame, not what a stage costs inside the stream of frames), medians over the frames behind two warm-up frames.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure(fn, reps, rounds, events=False):
    for _ in range(10):
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
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--latency-frames', type=int, default=6)
    a = ap.parse_args()
    from vilgod_amd import synthetic
    from vilgod_amd.frame_state import pack_clusters, pack_clusters_device, select_clusters_device
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from frame_latency import frame_latency
    dev = torch.device('cuda:0')
    host = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent')
    devp = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent', clip=host.clip, pack='device')
    poses = synthetic.make_poses(a.latency_frames + 4)
    names = ('pack.host', 'pack.device', 'pack.device_gpu', 'select.host', 'select.device', 'select.device_gpu')
    ms = {k: [] for k in names}
    spread = {k: [] for k in names}
    shape = {'points': [], 'clusters': [], 'packed_points': [], 'largest_cluster': [], 'valid_clusters': []}
    for f in range(a.frames):
        pts = synthetic.make_frame(1 + f, a.points, n_objects=a.objects)
        devp.new_sequence()
        fs, d_ref, d_X, gidx = devp.prepare(pts, poses[1], poses[0])
        d_labels, d_probs = devp.cluster(d_X)                 # pack='device': the hierarchy stage's CUDA tensors
        n = d_labels.numel()
        bound = n // devp.cluster_model.min_cluster_size + 1
        thr = devp.prob_threshold

        def pack_host():
            ids, index, seg = pack_clusters(d_labels.cpu().numpy(), d_probs.cpu().numpy(), thr)
            return ids, index, seg, torch.from_numpy(index).to(dev), torch.from_numpy(seg).to(dev)

        out = pack_clusters_device(d_labels, d_probs, thr, label_bound=bound)

        def pack_device():
            pack_clusters_device(d_labels, d_probs, thr, label_bound=bound, out=out)
            return out[3].cpu()

        ids, index, seg, d_index, d_seg = pack_host()
        C, P, over = (int(v) for v in pack_device())
        assert (C, P, over) == (len(ids), len(index), 0)
        assert np.array_equal(out[1][:P].cpu().numpy(), index) and np.array_equal(out[2][:C + 1].cpu().numpy(), seg)
        plane = devp.ground_plane(d_ref, gidx)
        valid, _ = devp.filter(d_X, d_index, d_seg, plane)

        def select_host():
            rows = np.flatnonzero(valid.cpu().numpy())
            parts = [index[seg[c]:seg[c + 1]] for c in rows]
            v_index = np.concatenate(parts) if parts else np.zeros(0, np.int32)
            v_seg = np.r_[0, np.cumsum([len(p) for p in parts])].astype(np.int32)
            return torch.from_numpy(v_index).to(dev), torch.from_numpy(v_seg).to(dev)

        sel = select_clusters_device(d_index, d_seg, C, valid, n_index=P)

        def select_device():
            select_clusters_device(d_index, d_seg, C, valid, n_index=P, out=sel)

        hv_index, hv_seg = select_host()
        select_device()
        K, Q = (int(v) for v in sel[2].cpu())
        assert torch.equal(sel[0][:Q], hv_index) and torch.equal(sel[1][:K + 1], hv_seg)
        runs = {'pack.host': (pack_host, False), 'pack.device': (pack_device, False), 'pack.device_gpu': (lambda: pack_clusters_device(
            d_labels, d_probs, thr, label_bound=bound, out=out), True), 'select.host': (select_host, False),
            'select.device': (select_device, False), 'select.device_gpu': (select_device, True)}
        for k, (fn, ev) in runs.items():
            med, lo, hi = _measure(fn, a.reps, a.rounds, events=ev)
            ms[k].append(med)
            spread[k].append((lo, hi))
        for k, v in (('points', n), ('clusters', C), ('packed_points', P), ('largest_cluster', int(np.diff(seg).max())), ('valid_clusters', K)):
            shape[k].append(v)
    frames = [torch.from_numpy(synthetic.make_frame(500 + i, a.points, n_objects=a.objects)).pin_memory() for i in range(a.latency_frames)]
    front = {}
    for name, pipe in (('host', host), ('device', devp)):
        med, tot = frame_latency(pipe, frames, poses)
        front[name] = {**med, 'total': tot,
                       'front_stage': round(sum(v for k, v in med.items() if k not in ('encode+scores', 'scores_d2h+box_wait', 'vote+results')), 3)}
    out = {'metric': 'cluster_pack_ms_per_frame', 'frames': a.frames, 'points_per_frame': a.points,
           'shape': {k: float(np.mean(v)) for k, v in shape.items()},
           'ms': {k: round(float(np.mean(v)), 4) for k, v in ms.items()},
           'ms_round_min_max': {k: [round(float(np.mean([s[0] for s in v])), 4), round(float(np.mean([s[1] for s in v])), 4)]
                                for k, v in spread.items()},
           'front_stage_ms': front, 'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
