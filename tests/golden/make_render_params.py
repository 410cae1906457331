"""Generates tests/golden/render_params_golden.npz: the REFERENCE's own renderer (stub-imported from the reference checkout, see
oracle/refstubs.py) at `lidar_image_projection` settings other than the shipped one.  Run only where the reference checkout exists:

    python tests/golden/make_render_params.py

Per setting, `mv_utils.RealisticProjection(cfg).get_img` and the resize / quantise lines of `ZeroShotDetector.classification`
(zero_shot_detector.py:405-409) run on five seeded clusters (10, 13, 49, ~400, ~3000 points).  The fixture is data: the clusters'
origin-transformed points, for the clusters under 50 points the reference's per-view `point_transform` output (it does not depend on the
setting, so it is stored once per cluster), and per (setting, cluster) the sha256 of the (R-2)^2 images and of the uint8 crops; the
arrays themselves for one cluster of every setting (the cluster changes from setting to setting), which keeps the file below the size
of render_golden.npz.  No reference source is stored.

Clusters under 50 points are meant to be rendered from the frozen view points through an identity view: torch-CPU multiplies such
small inputs without FMA (make_golden.py::make_render_small), and what is pinned here is everything downstream of that product.

The settings are the smallest at which a parameterised renderer can go wrong:
  R = 16            one accumulator per thread, a 14 -> 224 upsample, patch staging larger than both planes
  R = 97            odd row stride
  R = 111, 113      either side of the size at which the staged 224 x 224 bytes fit in the first plane
  R = 128           LDS and accumulator maximum
  D = 3             one usable slice, every value clipped to 1
  D = 32            the top bits of the 32-bit slice mask
  depth_bias = 0    slice 0 is reached, values clipped up to 1
  depth_bias = 1
  obj_ratio = 1.0   points on both clip borders
  obj_ratio = 0.3
  (96, 12, 0.7, 0.35) combined
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refstubs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# (resolution, depth, obj_ratio, depth_bias)
SETTINGS = [
    (16, 8, 0.8, 0.2), (97, 8, 0.8, 0.2), (111, 8, 0.8, 0.2), (113, 8, 0.8, 0.2), (128, 8, 0.8, 0.2),
    (112, 3, 0.8, 0.2), (112, 32, 0.8, 0.2), (112, 8, 0.8, 0.0), (112, 8, 0.8, 1.0),
    (112, 8, 1.0, 0.2), (112, 8, 0.3, 0.2), (96, 12, 0.7, 0.35),
]
CLUSTER_SIZES = [10, 13, 49, 397, 3011]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def clusters():
    """Seeded, roughly object shaped, float32 in the ego frame (as make_golden.py::render_cases)."""
    rng = np.random.default_rng(20250611)
    out = []
    for P, (az, rg) in zip(CLUSTER_SIZES, [(0.4, 7.0), (-1.2, 30.0), (2.6, 18.0), (1.1, 12.0), (-2.2, 42.0)]):
        c = np.array([rg * np.cos(az), rg * np.sin(az), 0.7])
        ext = rng.uniform([0.3, 0.3, 0.4], [2.2, 1.1, 1.0])
        out.append((rng.normal(size=(P, 3)) * ext + c).astype(np.float32))
    return out


def main():
    refstubs.install()
    from src.utils import mv_utils, pointcloud_utils
    store, hashes, stored = {}, [], []
    origins = []
    for k, pts in enumerate(clusters()):
        origin = pointcloud_utils.transform_cluster_points_to_origin(pts)          # pointcloud_utils.py:390
        t = torch.from_numpy(origin).float().unsqueeze(0)                           # zero_shot_detector.py:394
        origins.append(t)
        store[f'originf32_{k}'] = t[0].numpy()
    for s, (R, D, ratio, bias) in enumerate(SETTINGS):
        cfg = refstubs.projection_cfg()
        cfg.resolution, cfg.depth, cfg.obj_ratio, cfg.depth_bias = R, D, ratio, bias
        proj = mv_utils.RealisticProjection(cfg)
        if s == 0:
            store['rot_mat'] = proj.rot_mat.numpy()
        v = proj.translation.shape[0]
        for k, t in enumerate(origins):
            view_pts = proj.point_transform(points=torch.repeat_interleave(t, v, dim=0), rot_mat=proj.rot_mat.repeat(1, 1, 1))
            if t.shape[1] < 50:                                                     # frozen for the clusters that need them (see above)
                assert s == 0 or np.array_equal(store[f'viewpts_{k}'], view_pts.numpy())
                store[f'viewpts_{k}'] = view_pts.numpy()
            img = proj.get_img(t).detach()                                          # mv_utils.py:173
            assert img.shape == (v, 3, R - 2, R - 2)
            assert torch.equal(img[:, 0], img[:, 1]) and torch.equal(img[:, 0], img[:, 2])
            big = torch.nn.functional.interpolate(img, size=(224, 224), mode='bilinear', align_corners=True)
            big = big.permute(0, 3, 2, 1).detach().cpu().numpy()                    # zero_shot_detector.py:405-408
            u8 = np.stack([np.uint8(b * 255) for b in big])                         # :409
            assert (u8[..., 0] == u8[..., 1]).all() and (u8[..., 0] == u8[..., 2]).all()
            hashes.append([sha(img[:, 0].numpy()), sha(u8[..., 0])])
            if k == s % len(origins):                                               # arrays for one cluster per setting, hashes for all
                store[f'img_{s}_{k}'] = img[:, 0].numpy()
                store[f'u8_{s}_{k}'] = u8[..., 0]
                stored.append((s, k))
    store['settings'] = np.array(SETTINGS, dtype=np.float64)                       # the Python floats of the config, exactly
    store['hashes'] = np.array(hashes).reshape(len(SETTINGS), len(origins), 2)
    path = os.path.join(OUT, 'render_params_golden.npz')
    np.savez_compressed(path, **store)
    print('render_params_golden.npz', len(SETTINGS), 'settings x', len(origins), 'clusters,', len(stored), 'with arrays,',
          os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
