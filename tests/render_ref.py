"""Float32 restatement of the reference's renderer with the four `lidar_image_projection` numbers as arguments (TEST
INFRASTRUCTURE ONLY).  The same torch ops, in the same order, as oracle/render_oracle.py, which restates the shipped setting
(112, 8, 0.8, 0.2); tests/test_render_params_host.py pins this file against the reference's frozen outputs
(tests/golden/render_params_golden.npz) bit for bit, and the GPU tests use it as the reference for inputs the fixture does not hold.

Reference lines (paths relative to the reference checkout): src/utils/mv_utils.py:91-127 points2grid, :11-37 GridToImage,
src/vilgod/zero_shot_detector.py:405-409 resize / permute / uint8.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import render_oracle as ro


def points_to_grid(points, resolution, depth, obj_ratio, depth_bias):
    """mv_utils.py:91-127.  points: [B,P,3] float32 tensor -> [B,depth,R,R] (already permuted (0,1,3,2)).  obj_ratio and depth_bias
    are Python floats, `1 + depth_bias` is formed in double: torch rounds each scalar to float32 where it meets the tensor."""
    points = points.clone()
    batch = points.shape[0]
    pmax, pmin = points.max(dim=1)[0], points.min(dim=1)[0]
    pcent = ((pmax + pmin) / 2)[:, None, :]
    prange = (pmax - pmin).max(dim=-1)[0][:, None, None]
    points = (points - pcent) / prange * 2.
    points[:, :, :2] = points[:, :, :2] * obj_ratio
    _x = (points[:, :, 0] + 1) / 2 * resolution
    _y = (points[:, :, 1] + 1) / 2 * resolution
    _z = ((points[:, :, 2] + 1) / 2 + depth_bias) / (1 + depth_bias) * (depth - 2)
    _x.ceil_()
    _y.ceil_()
    z_int = _z.ceil()
    _x = torch.clip(_x, 1, resolution - 2)
    _y = torch.clip(_y, 1, resolution - 2)
    _z = torch.clip(_z, 1, depth - 2)
    coords = (z_int * resolution * resolution + _y * resolution + _x).long()
    grid = torch.zeros([batch, depth * resolution * resolution])
    grid.scatter_reduce_(1, coords, _z, 'amax', include_self=True)
    return grid.reshape(batch, depth, resolution, resolution).permute(0, 1, 3, 2)


def grid_to_image(grid, sigma=3.0):
    """mv_utils.py:30-37.  grid [B,depth,R,R] -> [B,3,R-2,R-2]."""
    x = F.max_pool3d(grid.unsqueeze(1), kernel_size=(1, 5, 5), stride=1, padding=(0, 1, 1))
    w = ro.gaussian_kernel_3x3(sigma).reshape(1, 1, 1, 3, 3)
    x = F.conv3d(x, w, bias=torch.zeros(1), stride=1, padding=(0, 1, 1))
    img = torch.max(x, dim=2)[0]
    img = img / torch.max(torch.max(img, dim=-1)[0], dim=-1)[0][:, :, None, None]
    img = 1 - img
    return img.repeat(1, 3, 1, 1)


def render_view_points(view_points, resolution, depth, obj_ratio, depth_bias):
    """From per-view points [V,P,3] (the output of point_transform): ([V,R-2,R-2] float32 images, uint8 crops [V,224,224]).
    V >= 2: the reference renders the views of a cluster as one batch (4 or more), and torch's CPU conv3d sums a batch of ONE in
    another order (last-bit differences in the image at every resolution, 112 included); that order is nobody's reference."""
    assert len(view_points) >= 2, 'a batch of one view is not what the reference evaluates'
    img = grid_to_image(points_to_grid(torch.as_tensor(view_points), resolution, depth, obj_ratio, depth_bias))
    u8 = ro.resize_quantise(img)
    return img[:, 0].numpy(), u8[..., 0]


def render_origin(origin_f32, resolution, depth, obj_ratio, depth_bias, rot=None):
    """From one cluster's origin-transformed points [P,3] float32, through the view product (mv_utils.py:173-201) on this host."""
    rot = ro.view_matrices() if rot is None else rot
    o = torch.as_tensor(origin_f32)
    pts = torch.matmul(torch.repeat_interleave(o.unsqueeze(0), rot.shape[0], dim=0), rot)
    return render_view_points(pts, resolution, depth, obj_ratio, depth_bias)


def setting(row):
    """A row of the fixture's `settings` array -> (resolution, depth, obj_ratio, depth_bias) with the config's Python types."""
    return int(row[0]), int(row[1]), float(row[2]), float(row[3])


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
