"""Encode rate of the CLIP image towers this project runs (ViT-B/16, ViT-B/32, ViT-L/14; clip_weights.TOWERS), fp16, synthetic
weights, f16 CHW crops (input kind 1, the path every non-patch-16 tower takes in the pipeline).  One JSON line per tower:

  encode_ms        median over 3 blocks of the mean encode time in the block (device events), after warm-up
  crops_per_s      crops / encode_ms
  tflops           shape-derived FLOPs / encode time: patch embedding + per block 2 T W (3W + W + 8W) + 4 T^2 W (attention), all T rows
                   of every block (the class-row-only last block does less: a lower bound on the rate)
  attn_us          mean time of one all-rows attention launch (vg_vit_profile_read_kind 2: HIP events around each launch, one encode)
  attn_floor_us    its byte floor: Q, K, V read once + O written (4 x n T W fp16) at 8 TB/s; attn_frac = floor / measured

    python tools/bench_clip_towers.py [--crops 328] [--towers ViT-B-16.pt,ViT-B-32.pt,ViT-L-14.pt] [--iters 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vilgod_amd import clip_weights as cw          # noqa: E402
from vilgod_amd.clip_wrapper import VitEncoder     # noqa: E402

HBM_BPS = 8e12


def tower_flops(cfg, n):
    W, L, p, res = cfg['width'], cfg['layers'], cfg['patch'], cfg['resolution']
    T = (res // p) ** 2 + 1
    f = 2.0 * (T - 1) * 3 * p * p * W                         # patch embedding (unpadded K)
    f += L * (2.0 * T * W * (3 * W + W + 8 * W) + 4.0 * T * T * W)
    f += 2.0 * W * cfg['output_dim']                          # head
    return n * f, T


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--crops', type=int, default=328)
    ap.add_argument('--towers', default=','.join(cw.TOWERS))
    ap.add_argument('--iters', type=int, default=5, help='encodes per timed block')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    for name in a.towers.split(','):
        cfg = cw.tower_config(name)
        wd = cw.synthetic_vit_weights(0, **cfg)
        enc = VitEncoder(wd, dtype='f16', device=dev)
        del wd
        x = torch.randn(a.crops, 3, cfg['resolution'], cfg['resolution'], generator=torch.Generator().manual_seed(0)).half().to(dev)
        for _ in range(3):
            enc.encode(x)
        torch.cuda.synchronize()
        blocks = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                enc.encode(x)
            e1.record()
            torch.cuda.synchronize()
            blocks.append(e0.elapsed_time(e1) / a.iters)
        ms = statistics.median(blocks)
        enc.profile(True)
        enc.encode(x)
        n_att, att_ms, _ = enc.profile_read(2)
        enc.profile(False)
        fl, T = tower_flops(cfg, a.crops)
        att_us = att_ms * 1e3 / max(n_att, 1)
        floor_us = 4.0 * a.crops * T * cfg['width'] * 2 / HBM_BPS * 1e6
        print(json.dumps({'tower': name, 'dtype': 'f16', 'crops': a.crops, 'tokens': T, 'encode_ms': round(ms, 3),
                          'encode_ms_blocks': [round(b, 3) for b in blocks], 'crops_per_s': round(a.crops / ms * 1e3, 1),
                          'tflops': round(fl / (ms * 1e-3) / 1e12, 1), 'attn_launches': n_att, 'attn_us': round(att_us, 1),
                          'attn_floor_us': round(floor_us, 1), 'attn_frac': round(floor_us / att_us, 3) if att_us else None}),
              flush=True)
        del enc, x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
