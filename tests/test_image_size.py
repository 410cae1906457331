"""`classification.image_size` other than 224 on the GPU: csrc/preprocess.hip through the C ABI (vg_clip_preprocess), the renderer's host
side and the classification stage.  The bar is byte equality throughout:
  1. the resample alone (in_kind 1) against tests/pil_ref.py and, through the frozen hashes, against PIL itself;
  2. the other output kinds as functions of the uint8 crop, as tests/test_render.py relates them for k_render;
  3. the whole chain (in_kind 0) against the reference's own chain, frozen as hashes (tests/golden/make_image_size.py);
  4. refused arguments launch nothing;
  5. render_frame / classify / the stage at 336, and the default path's bits around it.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pil_ref
from conftest import ROOT
from oracle import render_oracle as ro

GUARD = 4096          # bytes in front of and behind d_out
N_BYTES = {0: 224 * 224 * 3, 1: 3 * 224 * 224 * 4, 2: 3 * 224 * 224 * 2, 4: 196 * 768 * 2, 5: 196 * 256 * 2}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(f'{golden_dir}/image_size_golden.npz')


@pytest.fixture(scope='module')
def proj(cuda):
    from vilgod_amd.projection import RealisticProjection
    return RealisticProjection({}, device=cuda)


def _tables(S, dev):
    from vilgod_amd import pil_resample
    bounds, coef, ksize = pil_resample.bicubic_coeffs(S)
    return torch.from_numpy(bounds).to(dev), torch.from_numpy(coef).to(dev), ksize


def _preprocess(lut, d_in, in_kind, in_side, S, out_kind, tables=None, n=None):
    """vg_clip_preprocess into a guarded byte buffer -> (status, output bytes [n, bytes per crop], guards untouched)"""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    n = d_in.shape[0] if n is None else n
    bounds, coef, ksize = _tables(S, d_in.device) if tables is None else tables
    buf = torch.full((GUARD + n * N_BYTES[out_kind] + GUARD,), 0xA5, dtype=torch.uint8, device=d_in.device)
    body = buf[GUARD:GUARD + n * N_BYTES[out_kind]]
    st = lib.vg_clip_preprocess(ptr(d_in), in_kind, n, in_side, S, ptr(bounds), ptr(coef), ksize, ptr(lut), ptr(body), out_kind, stream_ptr())
    torch.cuda.synchronize()
    guards_ok = bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n * N_BYTES[out_kind]:] == 0xA5).all())
    return st, body.clone().reshape(n, N_BYTES[out_kind]), guards_ok


# ----------------------------------------------------------------------------------------------- 1. the resample alone
@pytest.mark.gpu
@pytest.mark.parametrize('family', pil_ref.RESAMPLE_FAMILIES)
@pytest.mark.parametrize('side', pil_ref.RESAMPLE_SIDES)
def test_resample_equals_pil(cuda, golden, proj, side, family):
    src = pil_ref.resample_inputs(side, family)
    want = pil_ref.resize_bicubic(src)
    assert pil_ref.sha(want) == golden['pil_hashes'][pil_ref.RESAMPLE_SIDES.index(side), pil_ref.RESAMPLE_FAMILIES.index(family)]
    st, out, guards_ok = _preprocess(proj._d_lut, torch.from_numpy(src).to(cuda), 1, 0, side, 0)
    assert st == 0 and guards_ok
    got = out.cpu().numpy().reshape(3, 224, 224, 3)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    print(f'side {side} {family}: bytes differing from PIL {int((got[..., 0] != want).sum())}/{want.size}')
    assert np.array_equal(got[..., 0], want)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[2], got[1])      # every crop from its own input


# ----------------------------------------------------------------------------------------------- 2. the output kinds
@pytest.mark.gpu
def test_output_kinds_are_functions_of_the_uint8_crop(cuda, proj):
    S = 336
    src = torch.from_numpy(pil_ref.resample_inputs(S, 'uniform')).to(cuda)
    n = src.shape[0]
    outs = {}
    for kind in (0, 1, 2, 4, 5):
        st, out, guards_ok = _preprocess(proj._d_lut, src, 1, 0, S, kind)
        assert st == 0 and guards_ok, kind
        outs[kind] = out.cpu()
    u8 = outs[0].numpy().reshape(n, 224, 224, 3)
    assert np.array_equal(u8[..., 0], pil_ref.resize_bicubic(src.cpu().numpy()))
    want = ro.clip_normalise(u8)                                                 # ToTensor + Normalize: [n,3,224,224] float32
    f32 = outs[1].view(torch.float32).reshape(n, 3, 224, 224)
    f16 = outs[2].view(torch.float16).reshape(n, 3, 224, 224)
    assert torch.equal(f32, want) and torch.equal(f16, want.half())
    p4 = outs[4].view(torch.float16).reshape(n * 196, 768)
    assert torch.equal(p4, f16.reshape(n, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(n * 196, 768))
    p5 = outs[5].view(torch.float16).reshape(n * 196, 256)
    level = (torch.from_numpy(u8[..., 0].copy()).float() / 256.0).reshape(n, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(n * 196, 256)
    assert torch.equal(p5.float(), level)


# ----------------------------------------------------------------------------------------------- 3. the whole chain
def _setting_proj(setting, dev):
    from vilgod_amd.projection import RealisticProjection
    R, D, ratio, bias = setting
    return RealisticProjection({'resolution': R, 'depth': D, 'obj_ratio': ratio, 'depth_bias': bias}, device=dev)


def _cluster(golden_dir, k, dev):
    o = np.load(f'{golden_dir}/render_params_golden.npz')[f'originf32_{k}']
    return torch.from_numpy(o).to(dev), torch.tensor([0, len(o)], dtype=torch.int32, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize('S', pil_ref.CHAIN_SIZES)
@pytest.mark.parametrize('s', range(len(pil_ref.CHAIN_SETTINGS)))
def test_chain_equals_the_reference(cuda, golden, golden_dir, s, S):
    p = _setting_proj(pil_ref.CHAIN_SETTINGS[s], cuda)
    assert np.array_equal(p.rot_mat.numpy(), np.load(f'{golden_dir}/render_params_golden.npz')['rot_mat'])
    for j, k in enumerate(pil_ref.CHAIN_CLUSTERS):
        pts, seg = _cluster(golden_dir, k, cuda)
        raw = p.render_origin(pts, seg, out='raw110')                             # [4, R-2, R-2]
        st, out, guards_ok = _preprocess(p._d_lut, raw, 0, p.image_side, S, 0)
        assert st == 0 and guards_ok
        got = out.cpu().numpy().reshape(4, 224, 224, 3)
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
        want = pil_ref.chain(raw.cpu().numpy(), S)
        print(f'setting {pil_ref.CHAIN_SETTINGS[s]} image_size {S} cluster {k}: bytes differing from the restatement '
              f'{int((got[..., 0] != want).sum())}/{want.size}')
        assert pil_ref.sha(got[..., 0]) == golden['chain_hashes'][s, pil_ref.CHAIN_SIZES.index(S), j], (s, S, k)


@pytest.mark.gpu
@pytest.mark.parametrize('s', range(len(pil_ref.CHAIN_SETTINGS)))
def test_chain_at_224_equals_the_renderers_own_crops(cuda, golden_dir, s):
    p = _setting_proj(pil_ref.CHAIN_SETTINGS[s], cuda)
    pts, seg = _cluster(golden_dir, pil_ref.CHAIN_CLUSTERS[0], cuda)
    raw = p.render_origin(pts, seg, out='raw110')
    want = p.render_origin(pts, seg, out='u8')
    st, out, guards_ok = _preprocess(p._d_lut, raw, 0, p.image_side, 224, 0)
    assert st == 0 and guards_ok and bool(want.any())
    assert torch.equal(out.reshape(4, 224, 224, 3), want)


# ----------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.gpu
def test_bad_arguments_launch_nothing(cuda, proj):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    src = torch.from_numpy(pil_ref.resample_inputs(448, 'uniform')).to(cuda)
    raw = torch.rand((3, 110, 110), device=cuda)

    def untouched(st, out, guards_ok):
        return st == 1 and guards_ok and bool((out == 0xA5).all())
    for S in (64, 449, 0, -336):
        assert untouched(*_preprocess(proj._d_lut, src, 1, 0, S, 0, tables=_tables(336, cuda))), S
    b, c, k = _tables(448, cuda)
    assert k == 9
    assert untouched(*_preprocess(proj._d_lut, src, 1, 0, 448, 0, tables=(b, c, 8)))              # short ksize
    assert untouched(*_preprocess(proj._d_lut, src, 1, 0, 448, 0, tables=(None, c, k)))
    assert untouched(*_preprocess(proj._d_lut, src, 1, 0, 448, 0, tables=(b, None, k)))
    assert untouched(*_preprocess(None, src, 1, 0, 448, 0))
    for kind in (3, 6, -1):
        buf = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=cuda)
        assert lib.vg_clip_preprocess(ptr(src), 1, 3, 0, 448, ptr(b), ptr(c), k, ptr(proj._d_lut), ptr(buf), kind, stream_ptr()) == 1
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all())
    for side in (13, 127):
        assert untouched(*_preprocess(proj._d_lut, raw, 0, side, 336, 0)), side
    assert untouched(*_preprocess(proj._d_lut, raw, 2, 110, 336, 0))
    out = torch.full((16,), 0xA5, dtype=torch.uint8, device=cuda)
    assert lib.vg_clip_preprocess(None, 1, 3, 0, 336, ptr(b), ptr(c), k, ptr(proj._d_lut), ptr(out), 0, stream_ptr()) == 1
    assert lib.vg_clip_preprocess(ptr(src), 1, 3, 0, 336, ptr(b), ptr(c), k, ptr(proj._d_lut), None, 0, stream_ptr()) == 1
    assert lib.vg_clip_preprocess(None, 1, 0, 0, 336, None, None, 0, None, None, 0, stream_ptr()) == 0      # nothing to do
    # a wider table than needed is fine: ksize is the row stride
    b7, c7, k7 = _tables(336, cuda)
    wide = torch.zeros((224, 12), dtype=torch.int32, device=cuda)
    wide[:, :k7] = c7
    src336 = torch.from_numpy(pil_ref.resample_inputs(336, 'binary')).to(cuda)
    st, out, guards_ok = _preprocess(proj._d_lut, src336, 1, 0, 336, 0, tables=(b7, wide, 12))
    assert st == 0 and guards_ok
    assert np.array_equal(out.cpu().numpy().reshape(3, 224, 224, 3)[..., 0], pil_ref.resize_bicubic(src336.cpu().numpy()))


# ----------------------------------------------------------------------------------------------- 5. host side and stage
def _frame(golden_dir, dev):
    g = np.load(f'{golden_dir}/render_golden.npz')
    clusters = [g[f'pts_{i}'] for i in range(g['hashes'].shape[0])]
    pts = np.concatenate(clusters).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int32)
    return torch.from_numpy(pts).to(dev), torch.from_numpy(seg).to(dev)


def _host_chain(raw, S):
    """kind 3 read back -> torch's CPU interpolate -> permute, uint8 -> tests/pil_ref.py: the reference's lines on this host"""
    img = raw.cpu()[:, None].repeat(1, 3, 1, 1)
    big = torch.nn.functional.interpolate(img, size=(S, S), mode='bilinear', align_corners=True).permute(0, 3, 2, 1).numpy()
    u8 = np.stack([np.uint8(b * 255) for b in big])[..., 0]
    return pil_ref.resize_bicubic(u8)


@pytest.mark.gpu
def test_render_frame_at_336_equals_the_host_chain_and_leaves_224_alone(cuda, golden_dir):
    from vilgod_amd.projection import RealisticProjection
    pts, seg = _frame(golden_dir, cuda)
    eye = np.eye(4)
    p = RealisticProjection({}, device=cuda)
    before = {o: p.render_frame(pts, None, seg, eye, out=o) for o in ('u8', 'f16', 'patch16c1')}
    u8 = p.render_frame(pts, None, seg, eye, out='u8', image_size=336)
    n = u8.shape[0]
    want = _host_chain(p.render_frame(pts, None, seg, eye, out='raw110', image_size=336), 336)
    assert torch.equal(u8[..., 0], u8[..., 1]) and torch.equal(u8[..., 0], u8[..., 2])
    assert np.array_equal(u8[..., 0].cpu().numpy(), want)
    assert not torch.equal(u8, before['u8'])
    assert list(p._pil_tables) == [336]                                        # the tables are kept per size
    p.render_frame(pts, None, seg, eye, out='u8', image_size=448)
    assert torch.equal(p.render_frame(pts, None, seg, eye, out='u8', image_size=336), u8) and sorted(p._pil_tables) == [336, 448]
    # the patch rows the tower takes, into a caller's buffer as the captured classifier passes one: rows beyond the crops untouched
    rows = p.render_frame(pts, None, seg, eye, out='patch16c1', image_size=336)
    level = (u8[..., 0].float() / 256.0).reshape(n, 14, 16, 14, 16).permute(0, 1, 3, 2, 4).reshape(n * 196, 256)
    assert torch.equal(rows[:n * 196].float(), level) and not rows[n * 196:].any()
    buf = torch.full((rows.shape[0] + 256, 256), 7.0, dtype=torch.float16, device=cuda)
    assert p.render_frame(pts, None, seg, eye, out='patch16c1', image_size=336, out_buf=buf) is buf
    assert torch.equal(buf[:n * 196], rows[:n * 196]) and bool((buf[n * 196:] == 7.0).all())
    # the default path afterwards: the bits of before, and of a projection that never saw another size
    fresh = RealisticProjection({}, device=cuda)
    for o, b in before.items():
        assert torch.equal(p.render_frame(pts, None, seg, eye, out=o), b), o
        assert torch.equal(fresh.render_frame(pts, None, seg, eye, out=o, image_size=224), b), o
    for size in (64, 449):
        with pytest.raises(NotImplementedError, match='image_size'):
            p.render_frame(pts, None, seg, eye, out='u8', image_size=size)


@pytest.mark.gpu
def test_classify_at_336_with_the_fp32_tower(cuda, golden_dir):
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pts, seg = _frame(golden_dir, cuda)
    eye = np.eye(4)
    pipe = PseudoLabelPipeline(device=cuda, vit_dtype='f32', max_points=24_000, clip_model_path='/nonexistent', box_workers=0)
    p224 = [t.clone() for t in pipe.classify(pts, None, seg, eye)]
    probs, top1, score = [t.clone() for t in pipe.classify(pts, None, seg, eye, image_size=336)]
    want_u8 = _host_chain(pipe.projection.render_frame(pts, None, seg, eye, out='raw110'), 336)
    crops = ro.clip_normalise(np.repeat(want_u8[..., None], 3, -1)).to(cuda).contiguous()
    hp, ht, hs = pipe.clip.predict_probs(crops)
    names = np.array(pipe.class_list, dtype=object)
    assert list(names[top1.cpu().numpy()]) == list(names[ht.cpu().numpy()])
    assert torch.equal(probs, hp) and torch.equal(score, hs)
    assert not torch.equal(probs, p224[0])                                      # another input than at 224
    # the pipeline's own setting, and the default path around it
    other = PseudoLabelPipeline(device=cuda, vit_dtype='f32', max_points=24_000, clip_model_path='/nonexistent', box_workers=0, clip=pipe.clip,
                                image_size=336)
    assert torch.equal(other.classify(pts, None, seg, eye)[0], probs)
    for a, b in zip(pipe.classify(pts, None, seg, eye), p224):
        assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match='image_size'):
        PseudoLabelPipeline(device=cuda, vit_dtype='f32', max_points=24_000, clip_model_path='/nonexistent', box_workers=0, clip=pipe.clip,
                            image_size=64)


STAGES = ['mask_ground_points', 'spatial_clustering', 'filter_detections', 'classification']


def _run_stage(root, *overrides):
    import pickle
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', 'pipeline_active=[' + ','.join(STAGES) + ']',
                          'pipeline.2.args.n_frames=1', 'dataset.SYNTHETIC.coherent=False', 'dataset.SYNTHETIC.frames_per_sequence=2',
                          'dataset.SYNTHETIC.points_per_frame=20000', 'dataset.SYNTHETIC.objects_per_frame=10',
                          'dataset.SYNTHETIC.n_sequences=1', 'end_sequence=0', 'device.max_points=24000', 'paths.clip_model=/nonexistent']
                         + list(overrides))
    with open(f'{root}/preprocessed_data/vilgod_mi355x_seq/synthetic_train_0000.pkl', 'rb') as f:
        return pickle.load(f)


@pytest.mark.gpu
def test_stage_at_336_fills_the_keys_it_fills_at_224(cuda, tmp_path):
    at224 = _run_stage(str(tmp_path / 'a'))
    at336 = _run_stage(str(tmp_path / 'b'), 'pipeline.5.args.image_size=336')
    key = 'clip_a_point_representation_of_a'
    n_classified = 0
    assert len(at224) == len(at336) == 2
    for x, y in zip(at224, at336):
        assert len(x['_detections']) == len(y['_detections'])
        for d, e in zip(x['_detections'], y['_detections']):
            assert set(d) == set(e) and d['valid'] == e['valid']
            assert set(d.get('object_class', {})) == set(e.get('object_class', {}))
            if key in d.get('object_class', {}):
                n_classified += 1
                assert len(e['object_class_predictions'][key]) == len(d['object_class_predictions'][key]) == 4
                assert len(e['object_class_predictions_score'][key]) == 4
    assert n_classified > 0
