"""`lidar_image_projection` at settings other than the shipped one, host side (no GPU).

  * tests/render_ref.py -- the float32 restatement of the reference's renderer with resolution, depth, obj_ratio and depth_bias as
    arguments -- reproduces every case of tests/golden/render_params_golden.npz (the reference's own outputs) bit for bit;
  * `RealisticProjection` accepts the ranges of vg_render_crops_ex and refuses, naming the key, what csrc/render.hip does not render;
  * a Hydra-style command-line override of the block reaches the projection object.
"""
import os

import numpy as np
import pytest
import torch

import render_ref as rr
from conftest import ROOT
from vilgod_amd import config as vconfig
from vilgod_amd import _lib
from vilgod_amd.projection import RealisticProjection

CFG = os.path.join(ROOT, 'tools', 'configs')
POOL = dict(_target_='torch.nn.MaxPool3d', kernel_size=(1, 5, 5), stride=1, padding=(0, 1, 1))
CONV = dict(_target_='torch.nn.Conv3d', in_channels=1, out_channels=1, kernel_size=(1, 3, 3), stride=1, padding=(0, 1, 1), bias=True)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(f'{golden_dir}/render_params_golden.npz')


def test_fixture_holds_the_cases_of_the_issue(golden):
    g = golden
    s = [rr.setting(r) for r in g['settings']]
    assert s == [(16, 8, 0.8, 0.2), (97, 8, 0.8, 0.2), (111, 8, 0.8, 0.2), (113, 8, 0.8, 0.2), (128, 8, 0.8, 0.2), (112, 3, 0.8, 0.2),
                 (112, 32, 0.8, 0.2), (112, 8, 0.8, 0.0), (112, 8, 0.8, 1.0), (112, 8, 1.0, 0.2), (112, 8, 0.3, 0.2), (96, 12, 0.7, 0.35)]
    sizes = [len(g[f'originf32_{k}']) for k in range(5)]
    assert sizes[:3] == [10, 13, 49] and 350 <= sizes[3] <= 450 and 2700 <= sizes[4] <= 3300
    assert g['hashes'].shape == (12, 5, 2)
    assert all(f'viewpts_{k}' in g for k in range(3))
    assert sum(k.startswith('img_') for k in g.files) == 12


def test_parameterised_restatement_matches_reference_golden(golden):
    """Every (setting, cluster): images and uint8 crops, sha256, and the arrays where the fixture holds them.  Clusters under 50 points
    from the reference's frozen view points (the FMA-or-not freedom of torch's small matmul), the others through this host's matmul."""
    g = golden
    rot = torch.from_numpy(g['rot_mat'])
    for s, row in enumerate(g['settings']):
        R, D, ratio, bias = rr.setting(row)
        for k in range(5):
            o = g[f'originf32_{k}']
            if len(o) < 50:
                img, u8 = rr.render_view_points(g[f'viewpts_{k}'], R, D, ratio, bias)
            else:
                img, u8 = rr.render_origin(o, R, D, ratio, bias, rot)
            assert img.shape == (4, R - 2, R - 2) and u8.shape == (4, 224, 224)
            assert [rr.sha(img), rr.sha(u8)] == list(g['hashes'][s, k]), (s, k)
            if f'img_{s}_{k}' in g:
                assert np.array_equal(img, g[f'img_{s}_{k}']) and np.array_equal(u8, g[f'u8_{s}_{k}'])


def test_restatement_at_the_shipped_setting_is_the_oracle(golden):
    from oracle import render_oracle as ro
    o = torch.from_numpy(golden['originf32_3'])
    want = ro.render_views(o)
    img, u8 = rr.render_origin(o, ro.RESOLUTION, ro.DEPTH, ro.OBJ_RATIO, ro.DEPTH_BIAS)
    assert np.array_equal(img, want[:, 0].numpy()) and np.array_equal(u8, ro.resize_quantise(want)[..., 0])


def test_cases_reach_the_edges_they_are_there_for(golden):
    """The fixture's clusters do reach what the settings are chosen for: slice 0 and values clipped up to 1 at depth_bias 0, the top
    slice at depth 32, one slice only at depth 3, both clip borders at obj_ratio 1."""
    g = golden
    vp = torch.from_numpy(g['viewpts_1'][1:2])             # the 13-point cluster, second view: its depth axis is the widest

    def slices(D, bias, pts=vp):
        grid = rr.points_to_grid(pts, 112, D, 0.8, bias)
        return [d for d in range(D) if grid[0, d].any()], grid
    occ, grid = slices(8, 0.0)
    assert 0 in occ and float(grid[0, 0].max()) == 1.0
    occ, _ = slices(32, 0.2)
    assert max(occ) == 30
    _, grid = slices(3, 0.2)
    assert set(np.unique(grid.numpy())) == {0.0, 1.0}
    grid = rr.points_to_grid(vp, 112, 8, 1.0, 0.2).amax(1)[0]
    rows, cols = torch.nonzero(grid.amax(1)).flatten(), torch.nonzero(grid.amax(0)).flatten()
    assert (int(rows.min()) == 1 and int(rows.max()) == 110) or (int(cols.min()) == 1 and int(cols.max()) == 110)


def test_render_kernels_use_no_scratch():
    """k_render and both k_render_ex instantiations keep their running maxima in registers (csrc/render.hip, the per-slice opaque thread id)."""
    from vilgod_amd import build
    assert build.check_scratch('render.hip', 'k_render') == []
    assert build.check_isa(sources=['render.hip']) == []


# ----------------------------------------------------------------------------------------------- constructor
def _cfg(**kw):
    c = dict(depth_bias=0.2, obj_ratio=0.8, bg_clr=0.0, resolution=112, depth=8, maxpool=dict(POOL), conv3d=dict(CONV),
             gaussian_kernel=dict(sigma=3, zsigma=1))
    c.update(kw)
    return c


def test_shipped_setting_keeps_the_specialised_kernel():
    for cfg in ({}, _cfg()):
        p = RealisticProjection(cfg, device='cpu')
        assert p._params is None and p.image_side == 110


@pytest.mark.parametrize('kw', [dict(resolution=16), dict(resolution=97), dict(resolution=128), dict(depth=3), dict(depth=32),
                                dict(obj_ratio=1.0), dict(obj_ratio=0.05), dict(depth_bias=0.0), dict(depth_bias=1.0),
                                dict(resolution=96, depth=12, obj_ratio=0.7, depth_bias=0.35)])
def test_projection_accepts_the_ranges(kw):
    p = RealisticProjection(_cfg(**kw), device='cpu')
    want = {**dict(resolution=112, depth=8, obj_ratio=0.8, depth_bias=0.2), **kw}
    assert (p.resolution, p.depth, p.obj_ratio, p.depth_bias) == tuple(want[k] for k in ('resolution', 'depth', 'obj_ratio', 'depth_bias'))
    assert p.image_side == want['resolution'] - 2
    q = p._params
    assert isinstance(q, _lib.RenderParams) and (q.resolution, q.depth) == (want['resolution'], want['depth'])
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert q.obj_ratio == f32(want['obj_ratio']) and q.depth_bias == f32(want['depth_bias'])
    # 1 + depth_bias: the double sum rounded once, which is what the float32 tensor meets at mv_utils.py:110
    assert q.one_plus_bias == f32(1 + want['depth_bias'])
    assert float((torch.ones(1) * 3) / (1 + want['depth_bias'])) == float(torch.tensor(3.0) / torch.tensor(q.one_plus_bias))


@pytest.mark.parametrize('key,kw', [
    ('resolution', dict(resolution=15)), ('resolution', dict(resolution=129)), ('resolution', dict(resolution=112.5)),
    ('depth', dict(depth=2)), ('depth', dict(depth=33)),
    ('obj_ratio', dict(obj_ratio=0.0)), ('obj_ratio', dict(obj_ratio=1.01)), ('obj_ratio', dict(obj_ratio=float('nan'))),
    ('depth_bias', dict(depth_bias=-0.1)), ('depth_bias', dict(depth_bias=1.5)),
    ('bg_clr', dict(bg_clr=1.0)),
    ('maxpool', dict(maxpool=dict(POOL, kernel_size=(1, 3, 3)))), ('maxpool', dict(maxpool=dict(POOL, stride=2))),
    ('maxpool', dict(maxpool=dict(POOL, padding=(0, 2, 2)))),
    ('conv3d', dict(conv3d=dict(CONV, kernel_size=(1, 5, 5)))), ('conv3d', dict(conv3d=dict(CONV, stride=(1, 2, 2)))),
    ('conv3d', dict(conv3d=dict(CONV, padding=0))),
])
def test_projection_refuses_by_key(key, kw):
    with pytest.raises(NotImplementedError, match=rf'lidar_image_projection\.{key}\b'):
        RealisticProjection(_cfg(**kw), device='cpu')


def test_cli_override_reaches_the_projection():
    c = vconfig.load(CFG, 'preprocessing', ['preprocessor=waymo', 'preprocessor.lidar_image_projection.resolution=96',
                                            'preprocessor.lidar_image_projection.obj_ratio=0.7'])
    p = RealisticProjection(c.preprocessor.lidar_image_projection, device='cpu')
    assert (p.resolution, p.depth, p.obj_ratio, p.depth_bias) == (96, 8, 0.7, 0.2)
    assert p._params is not None and p._params.resolution == 96 and p.image_side == 94
    # the shipped files, unmodified, stay on the specialised kernel
    for name in ('waymo', 'argoverse'):
        c = vconfig.load(CFG, 'preprocessing', [f'preprocessor={name}'])
        assert RealisticProjection(c.preprocessor.lidar_image_projection, device='cpu')._params is None
    with pytest.raises(NotImplementedError, match='resolution'):
        c = vconfig.load(CFG, 'preprocessing', ['preprocessor.lidar_image_projection.resolution=256'])
        RealisticProjection(c.preprocessor.lidar_image_projection, device='cpu')
