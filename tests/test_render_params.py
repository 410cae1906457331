"""The parameterised renderer (csrc/render.hip k_render_ex) through the C ABI, vg_render_crops_ex.

Bars:
  * every case of tests/golden/render_params_golden.npz (the reference's own renderer at twelve settings, five clusters each): the
    (R-2)^2 images (out_kind 3) and the uint8 crops (out_kind 0) equal the reference's frozen outputs BIT FOR BIT (sha256, arrays where
    stored).  Clusters under 50 points are rendered from the reference's frozen view points through an identity view (p @ I is exact;
    what that leaves open is the FMA-or-not of torch's small matmul, tests/golden/make_golden.py::make_render_small), the others
    from the origin points through the reference's view matrices.
  * at (112, 8, 0.8, 0.2) the parameterised kernel equals k_render (vg_render_crops) byte for byte in all six output kinds.
  * every crop slot is written by its own cluster through all three instantiations, at cluster counts on both sides of the 1024 up to
    which workgroups take the clusters largest first.
  * the other output kinds are functions of the uint8 crop, as tests/test_render.py relates them at 112.
  * settings outside the ranges are VG_ERR_ARG and write nothing.
  * the renderer -> tower hand-over of PseudoLabelPipeline.classify at a non-default setting.
"""
import ctypes

import numpy as np
import pytest
import torch

import render_ref as rr
from oracle import render_oracle as ro

IDENTITY = [(0.0, 0.0, 0.0)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(f'{golden_dir}/render_params_golden.npz')


def _pack(clusters, dev):
    pts = np.concatenate(clusters).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int32)
    return torch.from_numpy(pts).to(dev), torch.from_numpy(seg).to(dev)


def _out(kind, n, side, dev, fill=None):
    """Output buffer of vg_render_crops[_ex] for n crops; the patch-row kinds padded to the GEMM's 256-row tile."""
    rows = (n * 196 + 255) // 256 * 256
    shape, dt = {0: ((n, 224, 224, 3), torch.uint8), 1: ((n, 3, 224, 224), torch.float32), 2: ((n, 3, 224, 224), torch.float16),
                 3: ((n, side, side), torch.float32), 4: ((rows, 768), torch.float16), 5: ((rows, 256), torch.float16)}[kind]
    if fill is None:
        return torch.zeros(shape, dtype=dt, device=dev)
    return torch.full(shape, fill, dtype=dt, device=dev)


def _render_ex(proj, params, pts, seg, kind, out=None):
    """vg_render_crops_ex with the view matrices and the LUT of `proj` -> (status, output)."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    n = (seg.numel() - 1) * proj.num_views
    out = _out(kind, n, params.resolution - 2, pts.device) if out is None else out
    st = lib.vg_render_crops_ex(ptr(pts), ptr(seg), seg.numel() - 1, ptr(proj._d_rot), proj.num_views, ptr(proj._d_lut),
                                ctypes.byref(params) if params is not None else None, ptr(out), kind, stream_ptr())
    torch.cuda.synchronize()
    return st, out


def _frame_clusters(golden, n_extra=15, seed=5):
    """A frame-shaped input in the origin frame: the fixture's five clusters and seeded ones of 10 .. 6000 points (20 clusters)."""
    rng = np.random.default_rng(seed)
    clusters = [golden[f'originf32_{k}'] for k in range(5)]
    for P in [10, 11, 17, 33, 64, 65, 129, 250, 511, 700, 1024, 1025, 2000, 4100, 6000][:n_extra]:
        ext = rng.uniform([0.3, 0.3, 0.3], [3.0, 1.5, 2.0])
        clusters.append((rng.normal(size=(P, 3)) * ext + [0.0, 0.0, -1.0]).astype(np.float32))
    return clusters


# ----------------------------------------------------------------------------------------------- 1. the reference's frozen outputs
@pytest.mark.gpu
@pytest.mark.parametrize('s', range(12))
def test_hip_render_ex_matches_reference_golden_bit_exact(cuda, golden, s):
    from vilgod_amd._lib import RenderParams
    from vilgod_amd.projection import RealisticProjection
    g = golden
    R, D, ratio, bias = rr.setting(g['settings'][s])
    params = RenderParams(R, D, ratio, bias)
    views = RealisticProjection({}, device=cuda)
    assert np.array_equal(views.rot_mat.numpy(), g['rot_mat'])
    ident = RealisticProjection({}, device=cuda, views=IDENTITY)
    for k in range(5):
        o = g[f'originf32_{k}']
        if len(o) < 50:
            proj, (pts, seg) = ident, _pack(list(g[f'viewpts_{k}']), cuda)      # four "clusters" = the four frozen views
        else:
            proj, (pts, seg) = views, _pack([o], cuda)
        st, img = _render_ex(proj, params, pts, seg, 3)
        assert st == 0
        st, u8 = _render_ex(proj, params, pts, seg, 0)
        assert st == 0
        img, u8 = img.cpu().numpy(), u8.cpu().numpy()
        assert img.shape == (4, R - 2, R - 2) and (u8[..., 0] == u8[..., 1]).all() and (u8[..., 0] == u8[..., 2]).all()
        if f'img_{s}_{k}' in g:
            wi, wu = g[f'img_{s}_{k}'], g[f'u8_{s}_{k}']
            print(f'setting {s} {(R, D, ratio, bias)} cluster {k}: image values differing {int((img != wi).sum())}/{wi.size}, '
                  f'uint8 pixels differing {int((u8[..., 0] != wu).sum())}/{wu.size}')
            assert np.array_equal(img, wi) and np.array_equal(u8[..., 0], wu), (s, k)
        assert rr.sha(img) == g['hashes'][s, k, 0], (s, k)
        assert rr.sha(u8[..., 0]) == g['hashes'][s, k, 1], (s, k)


@pytest.mark.gpu
@pytest.mark.parametrize('setting', [(33, 5, 0.55, 0.6), (64, 4, 0.9, 0.1), (128, 16, 1.0, 0.0), (17, 32, 0.25, 1.0)])
def test_hip_render_ex_matches_the_restatement_on_other_settings(cuda, setting):
    """Settings the fixture does not hold, against tests/render_ref.py (pinned to the fixture by tests/test_render_params_host.py): a
    thin wall, a blob with coincident points and a 5000-point cluster, each seen from four sides by exact coordinate swaps and sign
    flips, already in view coordinates, through an identity view.  The restatement gets the four views of a cluster as one batch,
    as the reference renders them (a batch of one sums the convolution in another order, tests/render_ref.py)."""
    from vilgod_amd._lib import RenderParams
    from vilgod_amd.projection import RealisticProjection
    R, D, ratio, bias = setting
    rng = np.random.default_rng(R * 100 + D)
    wall = rng.uniform(-1, 1, size=(700, 3)) * [3.0, 0.02, 1.2]
    blob = np.repeat(rng.normal(size=(6, 3)) * [0.4, 0.4, 0.9], 3, axis=0)
    big = rng.normal(size=(5000, 3)) * [1.0, 2.0, 2.5]
    clusters = []
    for c in (wall, blob, big):
        c = c.astype(np.float32)
        clusters.append(np.stack([c, c[:, [1, 0, 2]], c * np.float32([-1.0, 1.0, -1.0]), c[:, [2, 1, 0]]]))   # [4,P,3] view points
    proj = RealisticProjection({}, device=cuda, views=IDENTITY)
    pts, seg = _pack([v for c in clusters for v in c], cuda)
    params = RenderParams(R, D, ratio, bias)
    st, img = _render_ex(proj, params, pts, seg, 3)
    assert st == 0
    st, u8 = _render_ex(proj, params, pts, seg, 0)
    assert st == 0
    img, u8 = img.cpu().numpy().reshape(3, 4, R - 2, R - 2), u8.cpu().numpy()[..., 0].reshape(3, 4, 224, 224)
    for i, c in enumerate(clusters):
        wi, wu = rr.render_view_points(c, R, D, ratio, bias)
        print(f'setting {setting} cluster {i}: image values differing {int((img[i] != wi).sum())}/{wi.size}, '
              f'uint8 pixels differing {int((u8[i] != wu).sum())}/{wu.size}')
        assert np.array_equal(img[i], wi), (setting, i)
        assert np.array_equal(u8[i], wu), (setting, i)


# ----------------------------------------------------------------------------------------------- 2. the shipped setting
@pytest.mark.gpu
@pytest.mark.parametrize('kind', range(6))
def test_hip_render_ex_at_the_shipped_setting_equals_render_crops(cuda, golden, kind):
    from vilgod_amd._lib import lib, ptr, stream_ptr, RenderParams
    from vilgod_amd.projection import RealisticProjection
    proj = RealisticProjection({}, device=cuda)
    clusters = _frame_clusters(golden)
    assert len(clusters) == 20
    pts, seg = _pack(clusters, cuda)
    n = len(clusters) * 4
    want = _out(kind, n, 110, cuda)
    assert lib.vg_render_crops(ptr(pts), ptr(seg), len(clusters), ptr(proj._d_rot), 4, ptr(proj._d_lut), ptr(want), kind, stream_ptr()) == 0
    st, got = _render_ex(proj, RenderParams(112, 8, 0.8, 0.2), pts, seg, kind)
    assert st == 0 and got.shape == want.shape
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert bool(want.any())


# ----------------------------------------------------------------------------------------------- 2b. which cluster a workgroup renders
SLOT_POOL_SIZES = [3, 17, 40, 17, 9, 40]                  # two pairs of equal size: a tie broken wrongly leaves a slot unwritten
SLOT_PATHS = {'fixed': None, 'ex12': (16, 8, 0.8, 0.2), 'ex16': (113, 8, 0.8, 0.2)}     # k_render, k_render_ex<12>, k_render_ex<16>


def _render_slots(path, proj, clusters, dev):
    """out_kind 3 of `clusters` through one of SLOT_PATHS into a NaN-filled buffer -> [C, side, side]"""
    from vilgod_amd._lib import lib, ptr, stream_ptr, RenderParams
    pts, seg = _pack(clusters, dev)
    setting = SLOT_PATHS[path]
    out = _out(3, len(clusters), (setting[0] if setting else 112) - 2, dev, fill=float('nan'))
    if setting is None:
        st = lib.vg_render_crops(ptr(pts), ptr(seg), len(clusters), ptr(proj._d_rot), 1, ptr(proj._d_lut), ptr(out), 3, stream_ptr())
        torch.cuda.synchronize()
    else:
        st, out = _render_ex(proj, RenderParams(*setting), pts, seg, 3, out=out)
    assert st == 0
    return out


@pytest.fixture(scope='module')
def slot_pool(cuda):
    """Six small point sets in view coordinates and, per path, each of them rendered alone (C = 1: the rank is trivially 0)."""
    from vilgod_amd.projection import RealisticProjection
    rng = np.random.default_rng(41)
    pool = [(rng.normal(size=(P, 3)) * rng.uniform(0.3, 2.0, size=3)).astype(np.float32) for P in SLOT_POOL_SIZES]
    assert not np.array_equal(pool[1], pool[3]) and not np.array_equal(pool[2], pool[5])
    proj = RealisticProjection({}, device=cuda, views=IDENTITY)
    alone = {path: torch.cat([_render_slots(path, proj, [m], cuda) for m in pool]) for path in SLOT_PATHS}
    for a in alone.values():
        assert bool(torch.isfinite(a).all()) and len({rr.sha(x.cpu().numpy()) for x in a}) == len(pool)      # six different images
    return proj, pool, alone


@pytest.mark.gpu
@pytest.mark.parametrize('C', [2, 7, 1024, 1025])
@pytest.mark.parametrize('path', list(SLOT_PATHS))
def test_hip_render_every_crop_slot_is_written_by_its_cluster(cuda, slot_pool, path, C):
    """The block-to-cluster choice of csrc/render.hip (render_block_cluster: rank by point count, ties to the lower index, label order
    above 1024 clusters) only decides WHEN a cluster is rendered: crop c is cluster c's image whatever the other clusters are.  Frames
    that cycle through the pool in a shuffled order -- 1024 is the last ranked count, 1025 the first in label order -- equal, byte for
    byte, the pool members rendered alone through the same entry point, and no slot keeps its NaN prefill."""
    proj, pool, alone = slot_pool
    order = np.random.default_rng(4).permutation(len(pool))
    member = order[np.arange(C) % len(pool)]
    assert SLOT_POOL_SIZES[member[0]] < SLOT_POOL_SIZES[member[1]]                   # label order is not rank order, already at C = 2
    got = _render_slots(path, proj, [pool[m] for m in member], cuda)
    assert not bool(torch.isnan(got).any())
    want = alone[path][torch.from_numpy(member).to(cuda)]
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------------------------- 3. the other output kinds
@pytest.mark.gpu
@pytest.mark.parametrize('R', [16, 97, 128])
def test_hip_render_ex_output_kinds_are_consistent(cuda, golden, R):
    """As tests/test_render.py relates them at 112: kinds 1 and 2 are the LUT of the uint8 crop (CHW, all three channels), kind 4 the
    im2col of kind 2 for 16 x 16 patches, kind 5 level / 256 of the uint8 crop in the same patch order; tile-padding rows untouched."""
    from vilgod_amd._lib import RenderParams
    from vilgod_amd.projection import RealisticProjection
    proj = RealisticProjection({}, device=cuda)
    clusters = _frame_clusters(golden, n_extra=6)
    pts, seg = _pack(clusters, cuda)
    n = len(clusters) * 4
    params = RenderParams(R, 8, 0.8, 0.2)
    res = {}
    for kind in (0, 1, 2, 4, 5):
        st, res[kind] = _render_ex(proj, params, pts, seg, kind)
        assert st == 0
    u8 = res[0]
    assert torch.equal(u8[..., 0], u8[..., 1]) and torch.equal(u8[..., 0], u8[..., 2])
    assert len(torch.unique(u8)) > 50                                               # a depth image, not a constant
    want = ro.clip_normalise(u8.cpu().numpy())
    assert torch.equal(res[1].cpu(), want)
    assert torch.equal(res[2].cpu(), want.half())
    im2col = res[2].reshape(n, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(n * 196, 768)
    assert res[4].shape[0] % 256 == 0 and torch.equal(res[4][:n * 196], im2col)
    assert not res[4][n * 196:].any()
    rows = (u8[..., 0].float() / 256.0).reshape(n, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(n * 196, 256)
    assert res[5].shape == ((n * 196 + 255) // 256 * 256, 256) and torch.equal(res[5][:n * 196].float(), rows)
    assert not res[5][n * 196:].any()


# ----------------------------------------------------------------------------------------------- 4. arguments
@pytest.mark.gpu
def test_hip_render_ex_rejects_settings_outside_the_ranges(cuda, golden):
    from vilgod_amd._lib import RenderParams
    from vilgod_amd.projection import RealisticProjection
    proj = RealisticProjection({}, device=cuda)
    pts, seg = _pack([golden['originf32_3']], cuda)

    def raw(R, D, ratio, bias, opb):
        p = RenderParams()
        p.resolution, p.depth, p.obj_ratio, p.depth_bias, p.one_plus_bias = R, D, ratio, bias, opb
        return p
    nan = float('nan')
    bad = [None, raw(15, 8, 0.8, 0.2, 1.2), raw(129, 8, 0.8, 0.2, 1.2), raw(-112, 8, 0.8, 0.2, 1.2), raw(112, 2, 0.8, 0.2, 1.2),
           raw(112, 33, 0.8, 0.2, 1.2), raw(112, 8, 0.0, 0.2, 1.2), raw(112, 8, 1.5, 0.2, 1.2), raw(112, 8, nan, 0.2, 1.2),
           raw(112, 8, 0.8, -0.1, 0.9), raw(112, 8, 0.8, 1.5, 2.5), raw(112, 8, 0.8, nan, 1.2), raw(112, 8, 0.8, 0.2, nan),
           raw(112, 8, 0.8, 0.2, 0.5)]
    for kind in (0, 3, 5):
        for p in bad:
            out = _out(kind, 4, 126, cuda, fill=7)
            st, out = _render_ex(proj, p, pts, seg, kind, out=out)
            assert st == 1, (kind, p and (p.resolution, p.depth, p.obj_ratio, p.depth_bias, p.one_plus_bias))
            assert bool((out == 7).all())                                            # nothing was launched
    # an empty frame does not make a bad setting acceptable; a good one is a no-op there
    empty = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert _render_ex(proj, raw(200, 8, 0.8, 0.2, 1.2), pts, empty, 0, out=_out(0, 1, 110, cuda))[0] == 1
    assert _render_ex(proj, RenderParams(96, 12, 0.7, 0.35), pts, empty, 0, out=_out(0, 1, 94, cuda))[0] == 0
    st, out = _render_ex(proj, RenderParams(96, 12, 0.7, 0.35), pts, seg, 6, out=_out(0, 4, 94, cuda, fill=7))
    assert st == 1 and bool((out == 7).all())
    st, out = _render_ex(proj, RenderParams(16, 3, 1.0, 0.0), pts, seg, 3)           # every lower bound at once is accepted
    assert st == 0 and out.shape == (4, 14, 14) and bool(torch.isfinite(out).all())
    st, out = _render_ex(proj, RenderParams(128, 32, 1.0, 1.0), pts, seg, 3)         # and every upper bound
    assert st == 0 and out.shape == (4, 126, 126) and bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------------------------- 5. host layer and hand-over
@pytest.mark.gpu
def test_projection_object_routes_by_setting(cuda, golden):
    """RealisticProjection at a non-default setting: render_frame / render_origin / get_img size their outputs from `resolution` and
    return what vg_render_crops_ex returns; at the shipped setting, what vg_render_crops returns."""
    from vilgod_amd._lib import RenderParams
    from vilgod_amd.projection import RealisticProjection
    o = golden['originf32_3']
    pts, seg = _pack([o], cuda)
    proj = RealisticProjection(dict(resolution=97, depth=8, obj_ratio=0.8, depth_bias=0.2), device=cuda)
    img = proj.get_img(torch.from_numpy(o).to(cuda)[None])
    assert img.shape == (4, 3, 95, 95) and torch.equal(img[:, 0], img[:, 2])
    assert rr.sha(img[:, 0].cpu().numpy()) == golden['hashes'][1, 3, 0]
    assert rr.sha(proj.render_origin(pts, seg, out='u8')[..., 0].cpu().numpy()) == golden['hashes'][1, 3, 1]
    ego = (np.random.default_rng(2).normal(size=(300, 3)) * [1.5, 0.7, 0.8] + [14.0, -6.0, 0.4]).astype(np.float32)
    d_ego, d_seg = _pack([ego], cuda)
    raw = proj.render_frame(d_ego, None, d_seg, np.eye(4), out='raw110')
    assert raw.shape == (4, 95, 95)
    _, want = _render_ex(proj, RenderParams(97, 8, 0.8, 0.2), proj._last['origin'], d_seg, 3)
    assert torch.equal(raw, want)


@pytest.mark.gpu
@pytest.mark.parametrize('single_channel', [False, True])
def test_pipeline_classifies_at_a_non_default_projection(cuda, golden, single_channel):
    """PseudoLabelPipeline.classify with lidar_image_projection = (96, 12, 0.7, 0.35): the config reaches the renderer, and the patch rows
    it hands to the tower are those of the SAME renderer's crops.  768-wide rows (patch_1ch off) are the im2col of the CHW fp16 crops
    (out_kind 2) and the tower computes the same numbers from either form (tests/test_render.py shows that at 112), so
    (probs, top1, score) equal clip_scores(encode(crops)) exactly.  The default single-channel rows go through the tower's folded
    K = 256 patch embedding, another summation than encode(crops) takes: they are compared exactly with the tower's result on rows
    built here from the out_kind 0 crop, and with the CHW result at 2e-3 on the probabilities -- both forms are fp16 evaluations of one
    tower, each held to 1e-3 of the fp32 oracle by tests/test_vit.py::test_hip_vit_b16_f16_error_on_rendered_crops."""
    from vilgod_amd.clip_wrapper import clip_scores
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    cfg['lidar_image_projection'] = dict(cfg['lidar_image_projection'], resolution=96, depth=12, obj_ratio=0.7, depth_bias=0.35)
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=20_000, clip_model_path='/nonexistent', box_workers=0,
                               box_mode='fast')
    pipe.patch_1ch = single_channel
    proj = pipe.projection
    assert (proj.resolution, proj.depth, proj.obj_ratio, proj.depth_bias) == (96, 12, 0.7, 0.35) and proj._params is not None
    assert pipe._clone_for_worker().projection._params.resolution == 96
    rng = np.random.default_rng(9)
    clusters = [(rng.normal(size=(P, 3)) * e + c).astype(np.float32) for P, e, c in
                [(12, (0.3, 0.3, 0.8), (9.0, 2.0, 0.5)), (300, (2.0, 0.8, 0.7), (-15.0, 6.0, 0.3)), (2500, (4.0, 1.2, 1.4), (25.0, -11.0, 0.9))]]
    d_X, d_seg = _pack(clusters, cuda)
    d_index = torch.arange(d_X.shape[0], dtype=torch.int32, device=cuda)
    T = np.eye(4)
    probs, top1, score = pipe.classify(d_X, d_index, d_seg, T)
    torch.cuda.synchronize()
    n = 12
    enc, text = pipe.clip.encoder, pipe.clip.text_features
    crops = proj.render_frame(d_X, d_index, d_seg, T, out='f16')
    assert crops.shape == (n, 3, 224, 224)
    p2, t2, s2 = clip_scores(enc.encode(crops), text)
    if not single_channel:
        assert torch.equal(probs, p2) and torch.equal(top1, t2) and torch.equal(score, s2)
    else:
        u8 = proj.render_frame(d_X, d_index, d_seg, T, out='u8')
        rows = torch.zeros(((n * 196 + 255) // 256 * 256, 256), dtype=torch.float16, device=cuda)
        rows[:n * 196] = (u8[..., 0].float() / 256.0).reshape(n, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(n * 196, 256).half()
        p1, t1, s1 = clip_scores(enc.encode_patches(rows, n), text)
        assert torch.equal(probs, p1) and torch.equal(top1, t1) and torch.equal(score, s1)
        perr = float((probs - p2).abs().max())
        print(f'single-channel rows vs CHW crops at (96, 12, 0.7, 0.35): max probability difference {perr:.2e}')
        assert perr <= 2e-3
    # the crops are those of the parameterised renderer, not of the shipped setting
    from vilgod_amd.projection import RealisticProjection
    other = RealisticProjection({}, device=cuda, angle_mode=proj.angle_mode).render_frame(d_X, d_index, d_seg, T, out='f16')
    assert not torch.equal(other, crops)
