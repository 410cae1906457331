"""Time of the class prompts' text features (CLIP.encode_text, model.py:343-356) by tower and number of prompts, one JSON line per case:

    python tools/bench_text_tower.py [--prompts 24 100 1203 4096] [--host-max 1203] [--threads 16] [--json profiles/text_tower_bench.json]

  host        clip_text.encode_text: plain torch on the CPU (`--threads` threads), what ClipWrapper(text='host') runs once at start-up.
              Timed once per size (no warm-up: that is how it runs), up to --host-max prompts.
  device_f32  clip_text.TextTower(dtype='f32').encode: vg_text_encode in chunks of 256 prompts, the parity mode
  device_f16  the same with dtype='f16'
at the ViT-B/16 text shapes (width 512, 12 layers, 8 heads, embed 512) and the ViT-L/14 text shapes (width 768, 12 layers, 12 heads,
embed 768), on seeded weights (clip_weights.synthetic_text_weights) and made-up token rows (sot, random ids, eot at a random position).
Device times: wall clock around encode + synchronize (tokens already on the host, features left on the device), three warm-up encodes,
then the median of five with min and max.  The handle's creation and weight upload are reported separately (`setup_s`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, ROUNDS = 3, 5
SHAPES = {'B/16': dict(width=512, layers=12, embed=512), 'L/14': dict(width=768, layers=12, embed=768)}
SOT, EOT = 49406, 49407


def make_tokens(n, seed=0, ctx=77):
    g = np.random.default_rng(seed)
    tok = np.zeros((n, ctx), np.int64)
    for r, e in enumerate(g.integers(3, 24, n)):            # prompt lengths of the shipped template: a handful of words
        tok[r, 0], tok[r, e] = SOT, EOT
        tok[r, 1:e] = g.integers(1, SOT, e - 1)
    return tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prompts', type=int, nargs='+', default=[24, 100, 1203, 4096])
    ap.add_argument('--host-max', type=int, default=1203)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--json', metavar='FILE', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                   'profiles', 'text_tower_bench.json'))
    a = ap.parse_args()
    from vilgod_amd import clip_text, clip_weights as cw
    torch.set_num_threads(a.threads)
    dev = torch.device('cuda:0')
    lines = []
    for name, shape in SHAPES.items():
        sd = cw.synthetic_text_weights(0, **shape)
        common = dict(bench='text_tower', device=torch.cuda.get_device_name(dev), tower=name, **shape, heads=shape['width'] // 64)
        for n in a.prompts:
            if n <= a.host_max:
                tok = make_tokens(n)
                t0 = time.perf_counter()
                clip_text.encode_text(sd, tok)
                lines.append(dict(common, mode='host', prompts=n, threads=a.threads, runs=1, s=round(time.perf_counter() - t0, 4)))
                print(json.dumps(lines[-1]), flush=True)
        for dtype in ('f32', 'f16'):
            t0 = time.perf_counter()
            tower = clip_text.TextTower(sd, dtype=dtype, device=dev)
            setup = time.perf_counter() - t0
            for n in a.prompts:
                tok = make_tokens(n)
                s = []
                for i in range(WARMUP + ROUNDS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tower.encode(tok)
                    torch.cuda.synchronize()
                    s.append(time.perf_counter() - t0)
                s = s[WARMUP:]
                lines.append(dict(common, mode='device_' + dtype, prompts=n, warmup=WARMUP, runs=ROUNDS, setup_s=round(setup, 4),
                                  s_median=round(float(np.median(s)), 5), s_min=round(min(s), 5), s_max=round(max(s), 5)))
                print(json.dumps(lines[-1]), flush=True)
            tower.close()
    if a.json:
        with open(a.json, 'w') as f:
            f.write(''.join(json.dumps(l) + '\n' for l in lines))


if __name__ == '__main__':
    main()
