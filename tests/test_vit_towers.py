"""CLIP image towers other than ViT-B/16, selected by `clip.model_name` (tools/configs/preprocessor/waymo.yaml, clip_utils.py:19):
ViT-B/32 (50 tokens, patch-embedding K = 3072) and ViT-L/14 (257 tokens: the flash-style k_attention_f16_long; K = 588, padded to
640).  ViT-L/14@336px is refused."""
import copy
import ctypes
import logging
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo
from vilgod_amd import clip_weights as cw, synthetic

VG_OK, VG_ERR_ARG = 0, 1
L14_SMALL = dict(width=1024, layers=2, heads=16, patch=14, resolution=224, output_dim=768)


def _clip_cfg(model_name):
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = copy.deepcopy(default_preprocessor_cfg())
    cfg['clip']['model_name'] = model_name
    return cfg


# ------------------------------------------------------------------------------------------- CPU
def test_tower_table_maps_the_model_names():
    assert cw.tower_config('ViT-B-16.pt') == cw.VIT_B16
    assert cw.tower_config('ViT-B-32.pt') == cw.VIT_B32 == dict(width=768, layers=12, heads=12, patch=32, resolution=224, output_dim=512)
    assert cw.tower_config('ViT-L-14.pt') == cw.VIT_L14 == dict(width=1024, layers=24, heads=16, patch=14, resolution=224, output_dim=768)
    assert cw.tower_config('RN50.pt') is None and cw.tower_config('my-finetune.pt') is None      # unknown -> the caller keeps B/16
    with pytest.raises(NotImplementedError, match='336'):
        cw.tower_config('ViT-L-14-336px.pt')
    for name, cfg in cw.TOWERS.items():
        assert cw.tower_name(cfg) == name
    assert cw.tower_name(L14_SMALL) is None


def test_clipwrapper_refuses_the_336px_tower():
    from vilgod_amd.clip_wrapper import ClipWrapper
    with pytest.raises(NotImplementedError, match='PIL'):
        ClipWrapper(_clip_cfg('ViT-L-14-336px.pt')['clip'], '/nonexistent', device='cpu')


def test_synthetic_l14_has_the_state_dict_shapes():
    wd = cw.synthetic_vit_weights(0, **cw.VIT_L14)
    assert wd['conv1.weight'].shape == (1024, 3, 14, 14)
    assert wd['positional_embedding'].shape == (257, 1024)
    assert wd['class_embedding'].shape == (1024,)
    assert wd['proj'].shape == (1024, 768)
    inp = [k for k in wd if k.endswith('attn.in_proj_weight')]
    assert len(inp) == 24 and all(wd[k].shape == (3072, 1024) for k in inp)
    assert cw.infer_config(wd) == cw.VIT_L14
    assert cw.infer_config(cw.synthetic_vit_weights(0, **dict(cw.VIT_B32, layers=1))) == dict(cw.VIT_B32, layers=1)


def test_long_attention_kernel_is_built_without_spills():
    from vilgod_amd import build
    asm = build._device_asm('vit.hip')
    assert 'k_attention_f16_long' in asm
    assert build.check_scratch('vit.hip', 'k_attention_f16_long') == []


def test_vit_create_limits():
    """vg_vit_create (no device work): the fp16 tower takes up to 1024 tokens and any patch size; the fp32 tower stops where
    k_attention_f32's rows no longer fit its 160 KiB of LDS (T <= 282)."""
    from vilgod_amd._lib import lib

    def create(width, heads, patch, res, dtype):
        h = ctypes.c_void_p()
        rc = lib.vg_vit_create(ctypes.byref(h), width, 1, heads, patch, res, 512, dtype)
        if rc == VG_OK:
            lib.vg_vit_destroy(h)
        return rc
    for dtype in (0, 1):
        assert create(1024, 16, 14, 224, dtype) == VG_OK          # ViT-L/14: 257 tokens, K = 588
        assert create(768, 12, 32, 224, dtype) == VG_OK           # ViT-B/32
        assert create(768, 12, 16, 224, dtype) == VG_OK           # ViT-B/16
    assert create(1024, 16, 14, 336, 1) == VG_OK                  # 577 tokens: fp16 only
    assert create(1024, 16, 14, 336, 0) == VG_ERR_ARG
    assert create(768, 12, 16, 16 * 16, 0) == VG_OK               # 257 tokens <= 282
    assert create(768, 12, 16, 16 * 17, 0) == VG_ERR_ARG          # 290 tokens
    assert create(768, 12, 7, 7 * 31, 1) == VG_OK                 # 962 tokens
    assert create(768, 12, 7, 7 * 32, 1) == VG_ERR_ARG            # 1025 tokens


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('n_crops,T,W,H', [(3, 257, 1024, 16), (4, 257, 768, 12), (1, 225, 768, 12), (2, 577, 1024, 16),
                                           (5, 1024, 768, 12)])
def test_hip_long_attention_alone(cuda, n_crops, T, W, H):
    """k_attention_f16_long through vg_attention against the float64 attention of the same fp16 inputs under the derived per-element
    bound of tests/attention_ref.py (as test_vit.py's test_hip_attention_alone), every row of every crop written, none beside them."""
    import attention_ref as R
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    ld = 3 * W + 64
    g = torch.Generator().manual_seed(T * 7 + n_crops)
    qkv = torch.zeros(n_crops * T, ld, dtype=torch.float16)
    qkv[:, :3 * W] = (torch.randn(n_crops * T, 3 * W, generator=g) * torch.tensor([1.5] * W + [1.0] * W + [2.0] * W)).half()
    d_qkv = qkv.to(cuda)
    buf = R.guarded_out(n_crops * T, W, torch.float16, cuda)
    check(lib.vg_attention(ptr(d_qkv), ctypes.c_void_p(buf.data_ptr() + W * 2), n_crops, T, W, H, ld, stream_ptr()))
    torch.cuda.synchronize()
    want, A = R.reference(qkv, n_crops, T, W, H)
    worst = R.check(buf, want, R.bound_f16(qkv, n_crops, T, W, H, want, A), n_crops, T)
    print(f'T={T} W={W}: worst |got - want| / bound = {worst:.3f}')


@pytest.mark.gpu
@pytest.mark.parametrize('tower', ['L14', 'B32'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_hip_tower_scores(cuda, tower, dtype):
    """The full synthetic tower on 6 crops, f32 and f16 CHW input (input kinds 0 / 1), against the fp32 oracle with the bounds of
    test_vit.py's test_hip_vit_b16_scores."""
    from vilgod_amd.clip_wrapper import VitEncoder, clip_scores
    cfg = cw.VIT_L14 if tower == 'L14' else cw.VIT_B32
    wd = cw.synthetic_vit_weights(0, **cfg)
    text = cw.synthetic_text_features(0, 24, cfg['output_dim'])
    x = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    enc = VitEncoder(wd, dtype=dtype, device=cuda)
    assert enc.cfg == cfg
    for xin in (x, x.half()):
        xo = xin.float()
        f_want, p_want = _oracle(wd, cfg['heads'], xo, text)
        f = enc.encode(xin.to(cuda))
        probs, top1, score = clip_scores(f, text.to(cuda))
        f, probs, top1 = f.cpu(), probs.cpu(), top1.cpu().numpy()
        idx_want, _ = vo.top1(p_want)
        rel = ((f - f_want).norm() / f_want.norm()).item()
        perr = (probs - p_want).abs().max().item()
        print(f'{tower} {dtype} input {xin.dtype}: feature rel L2 {rel:.2e}, max |dp| {perr:.2e}')
        assert torch.isfinite(f).all()
        if dtype == 'f32':
            assert perr < 1e-3
            assert np.array_equal(top1, idx_want)
        else:
            assert rel < 2e-2 and perr < 5e-2
            srt = np.sort(p_want.numpy(), axis=1)
            confident = (srt[:, -1] - srt[:, -2]) > 0.1
            assert np.array_equal(top1[confident], idx_want[confident])


def _oracle(wd, heads, x, text):
    with torch.no_grad():
        f = vo.vit_forward(wd, x, heads)
        return f, vo.clip_probabilities(f, text)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [3, 37])
def test_hip_l14_last_block_on_class_token_rows_only(cuda, n, monkeypatch):
    """The class-row-only last block launches k_attention_f16_long with one query tile: the features equal the all-rows run
    (VG_VIT_CLS_LAST=0) bit for bit, as test_vit.py's test_hip_last_block_on_class_token_rows_only asserts for ViT-B/16."""
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(2, **L14_SMALL)
    x = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).to(cuda)
    monkeypatch.setenv('VG_VIT_RESID_HL', '0')
    f_cls = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_VIT_CLS_LAST', '0')
    f_all = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    assert torch.isfinite(f_cls).all()
    assert torch.equal(f_cls, f_all), (f_cls - f_all).abs().max().item()


@pytest.mark.gpu
def test_hip_clipwrapper_synthetic_l14(cuda):
    from vilgod_amd.clip_wrapper import ClipWrapper
    cfg = _clip_cfg('ViT-L-14.pt')['clip']
    clip = ClipWrapper(cfg, '/nonexistent', device=cuda, dtype='f16')
    assert clip.encoder.cfg == cw.VIT_L14
    assert clip.weights_source == 'synthetic(seed=0, ViT-L-14.pt)'
    assert clip.text_features.shape == (len(cfg['class_list']), 768)
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(3)).half().to(cuda)
    probs, top1, score = clip.predict_probs(x)
    assert probs.shape == (5, len(cfg['class_list'])) and torch.isfinite(probs).all()
    b16 = ClipWrapper(_clip_cfg('ViT-B-16.pt')['clip'], '/nonexistent', device=cuda, dtype='f16')
    assert b16.weights_source == 'synthetic(seed=0)' and b16.encoder.cfg == cw.VIT_B16


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['state_dict', 'torchscript'])
def test_hip_clipwrapper_loads_an_l14_checkpoint(cuda, tmp_path, form):
    """A fabricated ViT-L-14.pt (the pattern of test_vit.py's test_hip_clipwrapper_loads_a_checkpoint_end_to_end): both forms load,
    the cached 768-d text features are used, the scores equal those of an encoder built directly from the tensors."""
    from vilgod_amd.clip_wrapper import ClipWrapper, VitEncoder, clip_scores
    wd = cw.synthetic_vit_weights(5, **cw.VIT_L14)
    half = {k: v.half() for k, v in wd.items()}
    sd = {**{'visual.' + k: v for k, v in half.items()},
          **{k: v.half() for k, v in cw.synthetic_text_weights(2, width=64, layers=1, embed=768).items()},
          'logit_scale': torch.tensor(4.6052)}
    ckpt = tmp_path / 'ViT-L-14.pt'
    if form == 'state_dict':
        torch.save(sd, ckpt)
    else:
        root = torch.nn.Module()
        for k, v in sd.items():
            parts, node = k.split('.'), root
            for p in parts[:-1]:
                if not hasattr(node, p):
                    node.add_module(p, torch.nn.Module())
                node = getattr(node, p)
            node.register_buffer(parts[-1], v)
        torch.jit.save(torch.jit.script(root), str(ckpt))
    cfg = _clip_cfg('ViT-L-14.pt')['clip']
    text = cw.synthetic_text_features(9, len(cfg['class_list']), 768)
    np.save(str(ckpt) + '.text_features.npy', text.numpy())
    clip = ClipWrapper(cfg, str(tmp_path), device=cuda, dtype='f16')
    assert clip.weights_source == str(ckpt) and clip.encoder.cfg == cw.VIT_L14
    x = (torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(2)) * 1.2).half().to(cuda)
    probs, top1, score = clip.predict_probs(x)
    del sd
    ref = VitEncoder({k: v.float() for k, v in half.items()}, dtype='f16', device=cuda)
    want = clip_scores(ref.encode(x), text.to(cuda))
    assert torch.equal(probs, want[0]) and torch.equal(top1, want[1])


@pytest.mark.gpu
def test_hip_pipeline_l14_matches_oracle_20k(cuda):
    """The 20k-point frame of test_pipeline.py's test_pipeline_matches_oracle_20k with `model_name: ViT-L-14.pt` in parity mode (fp32
    tower, CHW crops + im2col): every crop's probabilities within 1e-3 of the oracle's ViT-L/14, every name equal."""
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from oracle.pipeline_oracle import OraclePipeline
    cfg = _clip_cfg('ViT-L-14.pt')
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f32', max_points=25_000, clip_model_path='/nonexistent',
                               angle_mode='reference')
    assert pipe.clip.encoder.cfg == cw.VIT_L14 and 'ViT-L-14.pt' in pipe.clip.weights_source
    fs, res = pipe.process_frame(pts, poses[1], poses[0], fnr=1)
    wd = cw.synthetic_vit_weights(0, **cw.VIT_L14)
    text = cw.synthetic_text_features(0, 24, 768)
    orc = OraclePipeline(wd, text, cfg['clip']['class_list'], cfg['clip']['class_mapping'], heads=16, box_all_edges=False)
    o = orc.process_frame(pts, poses[1], poses[0])
    assert np.array_equal(fs.valid, o['valid'])
    got_p = pipe.last_probs.cpu().numpy()
    assert got_p.shape == o['probs_clip'].shape and got_p.shape[0] == 4 * int(o['valid'].sum()) > 0
    err = np.abs(got_p - o['probs_clip']).max()
    print('L/14 pipeline: valid', int(o['valid'].sum()), 'max |dp|', err)
    assert err < 1e-3
    e = fs.cls[pipe.cls_key]
    rows = np.flatnonzero(fs.valid)
    assert [str(e['name'][r]) for r in rows] == list(o['names'])
    assert set(res.keys()) == {'boxes_lidar', 'name', 'score', 'moving'}


@pytest.mark.gpu
@pytest.mark.parametrize('tower', ['complement', 'all'])
def test_hip_pipeline_l14_f16_full_size_frames(cuda, tower):
    """fp16 ViT-L/14 on 150k-point frames, several frames in flight on CU-masked ViT streams: finite probabilities, and the same
    outputs bit for bit as one frame at a time on unrestricted streams."""
    from vilgod_amd.pipeline import PseudoLabelPipeline
    cfg = _clip_cfg('ViT-L-14.pt')
    ref = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=160_000, clip_model_path='/nonexistent')
    assert ref.clip.encoder.cfg == cw.VIT_L14
    msk = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f16', max_points=160_000, clip_model_path='/nonexistent', clip=ref.clip,
                              cu_reserve=2, cu_tower=tower)
    poses = synthetic.make_poses(4)
    frames = [synthetic.make_frame(f, 150_000) for f in range(3)]
    ref.new_sequence(); msk.new_sequence()
    a = ref.process_frames([ref.upload(f) for f in frames], poses[1:4], poses[0], n_workers=3)
    b = msk.process_frames([msk.upload(f) for f in frames], poses[1:4], poses[0], n_workers=3)
    n_valid = 0
    for (fa, ra, pa), (fb, rb, pb) in zip(a, b):
        assert fa.valid.sum() > 10 and np.isfinite(ra['boxes_lidar']).all() and (ra['score'] > 0).all()
        assert torch.isfinite(pa).all() and pa.shape[1] == 24
        assert np.array_equal(fa.valid, fb.valid) and np.array_equal(pa.cpu().numpy(), pb.cpu().numpy())
        assert np.array_equal(ra['name'], rb['name']) and np.array_equal(ra['boxes_lidar'], rb['boxes_lidar'])
        n_valid += int(fa.valid.sum())
    assert n_valid > 30


@pytest.mark.gpu
def test_hip_cli_runs_the_l14_tower(cuda, tmp_path, caplog):
    """tools/preprocess_data.py with `preprocessor.clip.model_name=ViT-L-14.pt` on test_cli.py's synthetic sequence: it completes,
    its pickles have the ViT-B/16 run's keys and layout, and the log names the tower."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    from test_cli import OVR, _load
    outs = {}
    for name in ('ViT-B-16.pt', 'ViT-L-14.pt'):
        root = str(tmp_path / name)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', f'preprocessor.clip.model_name={name}'] + OVR)
        outs[name] = (_load(root), caplog.text)
    (res_b, idx_b, st_b), log_b = outs['ViT-B-16.pt']
    (res_l, idx_l, st_l), log_l = outs['ViT-L-14.pt']
    assert 'CLIP tower: ViT-B-16.pt' in log_b and 'synthetic(seed=0)' in log_b
    assert 'CLIP tower: ViT-L-14.pt (width 1024, layers 24, patch 14' in log_l and 'synthetic(seed=0, ViT-L-14.pt)' in log_l
    assert idx_l == idx_b and len(res_l) == len(res_b) == 6 and len(st_l) == len(st_b)
    for fb, fl in zip(res_b, res_l):
        assert set(fl) == set(fb)
        for k in fb:
            assert type(fl[k]) is type(fb[k])
            if isinstance(fb[k], np.ndarray):
                # (a frame's score array is float32 or float64 with its data, as upstream: np.array over numpy float32 / python floats)
                assert fl[k].dtype.kind == fb[k].dtype.kind and fl[k].shape[1:] == fb[k].shape[1:]
    key = 'clip_a_point_representation_of_a'
    for sb, sl in zip(st_b, st_l):
        assert set(sl) == set(sb)
        for d in sl['_detections']:
            if d['valid']:
                assert key in d['object_class'] and len(d['object_class_predictions'][key]) == 4
    assert pickle.dumps(res_l)      # plain picklable data
