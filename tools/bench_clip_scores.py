"""GPU time of the scores head (clip_utils.py:42-61) by length of clip.class_list, one JSON line:

    python tools/bench_clip_scores.py [--crops 328] [--reps 50] [--rounds 5] [--json FILE]

  narrow   vg_clip_scores: one wave per crop, up to 64 classes (what the shipped 24-class list runs)
  wide     vg_clip_scores_wide: one 256-thread workgroup per crop, any number of classes (what longer lists run)
for feature widths 512 (ViT-B) and 768 (ViT-L/14) and 24 (both kernels), 65, 256, 1203 and 4096 classes, on seeded unit rows.
GPU times are HIP event pairs around `reps` back-to-back launches, after 10 warm-up launches; the median of `rounds` such measurements
with their min / max.  Each time is also given as a share of one fp16 vg_vit_encode of the same crops (ViT-B/16 for 512, ViT-L/14 for
768, seeded synthetic weights, timed the same way with --encode-reps launches per round).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP = 10
CLASSES = (24, 65, 256, 1203, 4096)


def _time(fn, reps, rounds, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return dict(us_median=round(float(np.median(ms)) * 1e3, 2), us_min=round(min(ms) * 1e3, 2), us_max=round(max(ms) * 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crops', type=int, default=328)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--encode-reps', type=int, default=5)
    ap.add_argument('--no-encode', action='store_true', help='skip the vg_vit_encode timings (no shares)')
    ap.add_argument('--json', metavar='FILE', default=None)
    a = ap.parse_args()
    from vilgod_amd import clip_weights as cw
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    from vilgod_amd.clip_wrapper import VitEncoder, NARROW_CLASSES
    dev = torch.device('cuda:0')
    n = a.crops
    out = dict(bench='clip_scores', device=torch.cuda.get_device_name(dev), crops=n, warmup=WARMUP, rounds=a.rounds,
               launches_per_round=a.reps, dims={})
    for dim, tower in ((512, cw.VIT_B16), (768, cw.VIT_L14)):
        g = torch.Generator().manual_seed(dim)
        feat = torch.randn(n, dim, generator=g).to(dev)
        res = {}
        enc_us = None
        if not a.no_encode:
            enc = VitEncoder(cw.synthetic_vit_weights(0, **tower), dtype='f16', device=dev)
            r = enc.cfg['resolution']
            crops = (torch.randn(n, 3, r, r, generator=g) * 0.8).half().to(dev)
            t = _time(lambda: enc.encode(crops), a.encode_reps, a.rounds, warmup=2)
            enc_us = t['us_median']
            res['vit_encode'] = dict(t, launches_per_round=a.encode_reps)
            del enc, crops
        for K in CLASSES:
            text = torch.randn(K, dim, generator=g)
            text = (text / text.norm(dim=-1, keepdim=True)).to(dev)
            probs = torch.empty((n, K), dtype=torch.float32, device=dev)
            top1 = torch.empty((n,), dtype=torch.int32, device=dev)
            score = torch.empty((n,), dtype=torch.float32, device=dev)
            for name, fn in (('narrow', lib.vg_clip_scores), ('wide', lib.vg_clip_scores_wide)):
                if name == 'narrow' and K > NARROW_CLASSES:
                    continue
                t = _time(lambda: check(fn(ptr(feat), n, dim, ptr(text), K, ptr(probs), ptr(top1), ptr(score), stream_ptr()), name),
                          a.reps, a.rounds)
                if enc_us:
                    t['share_of_vit_encode'] = round(t['us_median'] / enc_us, 5)
                res[f'{name}_{K}'] = t
        out['dims'][str(dim)] = res
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
