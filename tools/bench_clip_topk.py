"""Top-k class selection on the GPU beside what it replaces, one JSON line (also written to profiles/clip_topk_bench.json):

    python tools/bench_clip_topk.py [--crops 328] [--reps 50] [--rounds 5] [--out profiles/clip_topk_bench.json]

328 crops (a frame's worth), D = 512, class lists of 24 / 100 / 1203 / 4096 seeded unit text rows, top_k = 2 / 5 / 16.  Per case:
  topk_gpu_us     vg_clip_topk alone, pre-allocated outputs, `reps` back-to-back launches between two HIP events
  scores_gpu_us   the vg_clip_scores / vg_clip_scores_wide launch in front of it, measured the same way (once per class list)
  host_ms         what the selection would cost on the host: the [crops, classes] table copied down (stream drained) plus the
                  reference's per-row np.argpartition / np.argsort loop (clip_utils.py:51-61), wall time; `copy_ms` is the copy alone
10 warm-up launches, then the median of `rounds` measurements with their min and max.  `equal`: the kernel's indices are the host
loop's for every row (seeded softmax rows have no ties where the cut falls).  Not measured here: the pipeline's frame rate.
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


def _stats(out, digits=3):
    return {'median': round(float(np.median(out)), digits), 'min': round(float(min(out)), digits), 'max': round(float(max(out)), digits)}


def _events(fn, reps, rounds, warmup=10):
    """microseconds per launch"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / reps)
    return _stats(out, 2)


def host_topk(table, k):
    """the per-row loop of clip_utils.py:51-61 -> indices [n, k]"""
    idx = np.empty((len(table), k), np.int64)
    for i in range(len(table)):
        row = table[i, :]
        top = np.argpartition(row, -k)[-k:]
        idx[i] = top[np.argsort(-row[top])]
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crops', type=int, default=328)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_topk_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import clip_weights as cw
    from vilgod_amd.clip_wrapper import clip_scores, clip_topk
    torch.set_num_threads(1)
    dev = torch.device('cuda:0')
    n, D = a.crops, 512
    feat = (torch.randn(n, D, generator=torch.Generator().manual_seed(0)) * 1.3).to(dev)
    res = {'metric': 'clip_topk_us_per_launch', 'crops': n, 'dim': D, 'cases': {}}
    for K in (24, 100, 1203, 4096):
        text = cw.synthetic_text_features(K, K, D).to(dev)
        probs = clip_scores(feat, text)[0]
        scores_us = _events(lambda: clip_scores(feat, text), a.reps, a.rounds)
        copy_ms = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = probs.cpu().numpy()
            copy_ms.append(1e3 * (time.perf_counter() - t0))
        for k in (2, 5, 16):
            top = torch.empty((n, k), dtype=torch.int32, device=dev)
            score = torch.empty((n, k), dtype=torch.float32, device=dev)
            topk_us = _events(lambda: clip_topk(probs, k, top, score), a.reps, a.rounds)
            host_ms = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want = host_topk(probs.cpu().numpy(), k)
                host_ms.append(1e3 * (time.perf_counter() - t0))
            res['cases'][f'K{K}_k{k}'] = {'classes': K, 'top_k': k, 'equal': bool(np.array_equal(top.cpu().numpy(), want)),
                                          'topk_gpu_us': topk_us, 'scores_gpu_us': scores_us, 'host_ms': _stats(host_ms),
                                          'copy_ms': _stats(copy_ms), 'table_bytes': int(table.nbytes)}
    res.update({'reps': a.reps, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(dev)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
