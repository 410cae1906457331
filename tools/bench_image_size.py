"""GPU time per frame of the crops at `classification.image_size` other than 224 on the benchmark's frame shape (one synthetic
150k-point frame with 60 objects, its valid clusters x 4 views, single-channel fp16 patch rows = the product hand-over):

  size_224             k_render alone (vg_render_crops writes the patch rows itself): the shipped path
  size_112 / 336 / 448 k_render into its raw 110 x 110 images (out_kind 3), then k_clip_preprocess (vg_clip_preprocess, csrc/preprocess.hip)
                       into the patch rows (`frame`); `preprocess` is the second launch alone

Per variant: 10 warm-up launches, then 5 rounds of `--launches` launches between two events; the median round with min / max, in
microseconds per frame.  The origin transform runs once, in front.  Prints one JSON line per variant, which is what
profiles/image_size_bench.json holds.

    python tools/bench_image_size.py [--points 150000] [--objects 60] [--launches 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vilgod_amd import synthetic  # noqa: E402
from vilgod_amd._lib import lib, ptr, stream_ptr, check  # noqa: E402
from vilgod_amd.frame_state import pack_clusters  # noqa: E402
from vilgod_amd.pipeline import PseudoLabelPipeline  # noqa: E402
from vilgod_amd.projection import OUT_PATCH16_1CH, OUT_RAW110  # noqa: E402

WARMUP, ROUNDS = 10, 5
SIZES = [224, 112, 336, 448]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=150_000)
    ap.add_argument('--objects', type=int, default=60)
    ap.add_argument('--seed', type=int, default=300)
    ap.add_argument('--launches', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    pipe = PseudoLabelPipeline(device=dev, max_points=a.points + 1024, clip_model_path='/nonexistent', box_workers=0)
    poses = synthetic.make_poses(3)
    pts = pipe.upload(synthetic.make_frame(a.seed, a.points, n_objects=a.objects))
    fs, d_ref, d_X, gidx = pipe.prepare(pts, poses[1], poses[0], fnr=0)
    labels, pr = pipe.cluster(d_X)
    ids, index, seg = pack_clusters(labels, pr, pipe.prob_threshold)
    d_index, d_seg = torch.from_numpy(index).to(dev), torch.from_numpy(seg).to(dev)
    valid, _ = pipe.filter(d_X, d_index, d_seg, pipe.ground_plane(d_ref, gidx))
    vrows = np.flatnonzero(valid.cpu().numpy())
    parts = [index[seg[c]:seg[c + 1]] for c in vrows]
    d_vi = torch.from_numpy(np.concatenate(parts)).to(dev)
    d_vs = torch.from_numpy(np.r_[0, np.cumsum([len(p) for p in parts])].astype(np.int32)).to(dev)
    proj = pipe.projection
    proj.render_frame(d_X, d_vi, d_vs, fs.transform_to_ego, out='patch16c1')
    origin = proj._last['origin']
    C, V = len(vrows), proj.num_views
    n = C * V
    out = torch.zeros(((n * 196 + 255) // 256 * 256, 256), dtype=torch.float16, device=dev)
    raw = torch.zeros((n, proj.image_side, proj.image_side), dtype=torch.float32, device=dev)
    sp = stream_ptr()

    def render(target, kind):
        check(lib.vg_render_crops(ptr(origin), ptr(d_vs), C, ptr(proj._d_rot), V, ptr(proj._d_lut), ptr(target), kind, sp), 'vg_render_crops')

    def preprocess(size):
        bounds, coef, ksize = proj._resample_tables(size, dev)
        check(lib.vg_clip_preprocess(ptr(raw), 0, n, proj.image_side, size, ptr(bounds), ptr(coef), ksize, ptr(proj._d_lut), ptr(out),
                                     OUT_PATCH16_1CH, sp), 'vg_clip_preprocess')

    def timed(launch):
        for _ in range(WARMUP):
            launch()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / a.launches * 1000.0)
        rounds.sort()
        return dict(us_median=round(rounds[ROUNDS // 2], 2), us_min=round(rounds[0], 2), us_max=round(rounds[-1], 2))

    common = dict(bench='image_size', device=torch.cuda.get_device_name(0), points=a.points, objects=a.objects, seed=a.seed, clusters=int(C),
                  views=int(V), out_kind='patch16c1', warmup=WARMUP, rounds=ROUNDS, launches_per_round=a.launches)
    for size in SIZES:
        if size == 224:
            res = dict(image_size=224, path='k_render', frame=timed(lambda: render(out, OUT_PATCH16_1CH)))
        else:
            render(raw, OUT_RAW110)
            res = dict(image_size=size, path='k_render (raw) + k_clip_preprocess',
                       frame=timed(lambda: (render(raw, OUT_RAW110), preprocess(size))), preprocess=timed(lambda: preprocess(size)))
        print(json.dumps(dict(common, **res)), flush=True)


if __name__ == '__main__':
    main()
