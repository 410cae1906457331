"""CLIP ViT image tower + scoring parity.

CPU:  oracle/vit_oracle.py == the reference's VisionTransformer outputs frozen in tests/golden/vit_golden.npz
      (reduced config with stored weights-by-seed, and the full ViT-B/16 regenerated from seed 0).
GPU:  csrc/vit.hip through the C ABI.
      fp32 mode: probabilities within 1e-3 of the oracle, identical top-1 (north_star tolerance).
      fp16 mode: throughput mode (what the reference itself runs on a GPU); tolerance is necessarily looser:
                 features within 2e-2 relative L2, probabilities within 5e-2, top-1 equal wherever the oracle's
                 top-2 margin exceeds 0.1.
"""
import os

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo
from vilgod_amd import clip_weights as cw

TOL_PROB_F32 = 1e-3


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(f'{golden_dir}/vit_golden.npz')


def small_cfg(g):
    keys = ('width', 'layers', 'heads', 'patch', 'resolution', 'output_dim')
    return dict(zip(keys, [int(v) for v in g['cfg']]))


# ------------------------------------------------------------------------------------------- CPU
def test_oracle_matches_reference_small(golden):
    cfg = small_cfg(golden)
    wd = cw.synthetic_vit_weights(int(golden['seed']), **cfg)
    y = vo.vit_forward(wd, torch.from_numpy(golden['x']), cfg['heads'])
    assert np.abs(y.numpy() - golden['y']).max() < 2e-5


def test_oracle_matches_reference_vit_b16(golden):
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    xb = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(int(golden['xb_seed'])))
    with torch.no_grad():
        y = vo.vit_forward(wd, xb, 12)
    assert np.abs(y.numpy() - golden['yb']).max() < 5e-5


def test_weight_names_match_reference_state_dict():
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    assert sum(v.numel() for v in wd.values()) == 86192640          # SURVEY §8c [probe]
    assert cw.infer_config(wd) == cw.VIT_B16
    assert wd['transformer.resblocks.11.attn.in_proj_weight'].shape == (2304, 768)


def test_vote_ties_and_majority():
    names = np.array(['Vehicle', 'Vehicle', 'Pedestrian', 'Background'])
    assert vo.vote(names, np.array([0.5, 0.7, 0.9, 0.2]))[0] == 'Vehicle'
    names = np.array(['Vehicle', 'Vehicle', 'Pedestrian', 'Pedestrian'])
    n, s = vo.vote(names, np.array([0.5, 0.7, 0.9, 0.2]))
    assert n == 'Vehicle' and abs(s - 0.6) < 1e-12      # tie -> best mean score (0.6 vs 0.55)
    n, s = vo.vote(names, np.array([0.5, 0.5, 0.6, 0.4]))
    assert n == 'Pedestrian' or n == 'Vehicle'


# ------------------------------------------------------------------------------------------- GPU
def _oracle_probs(wd, heads, x, text):
    with torch.no_grad():
        f = vo.encode_in_chunks(wd, x, heads, 50)
        return f, vo.clip_probabilities(f, text)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 6, 9])
def test_hip_vit_small_f32(cuda, golden, n):
    from vilgod_amd.clip_wrapper import VitEncoder, clip_scores
    cfg = small_cfg(golden)
    wd = cw.synthetic_vit_weights(int(golden['seed']), **cfg)
    x = torch.from_numpy(golden['x'])
    x = torch.cat([x, x.flip(0)])[:n].contiguous() if n > 6 else x[:n].contiguous()
    enc = VitEncoder(wd, dtype='f32', device=cuda)
    f = enc.encode(x.to(cuda)).cpu()
    want = vo.vit_forward(wd, x, cfg['heads'])
    if n <= 6:
        assert np.abs(f.numpy()[:n] - golden['y'][:n]).max() < 5e-5     # vs the reference's own output
    assert (f - want).abs().max() < 5e-5


@pytest.mark.gpu
def test_hip_vit_small_f16(cuda, golden):
    from vilgod_amd.clip_wrapper import VitEncoder
    cfg = small_cfg(golden)
    wd = cw.synthetic_vit_weights(int(golden['seed']), **cfg)
    x = torch.from_numpy(golden['x'])
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    f = enc.encode(x.to(cuda)).cpu()
    f_h = enc.encode(x.half().to(cuda)).cpu()
    want = torch.from_numpy(golden['y'])
    rel = ((f - want).norm() / want.norm()).item()
    print('small f16 rel L2 err', rel)
    assert rel < 1e-2
    assert ((f_h - want).norm() / want.norm()).item() < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f16', 'f16-resid16'])
def test_hip_vit_b16_scores(cuda, dtype, monkeypatch):
    """Full ViT-B/16, seeded synthetic weights, 10 crops (one more than a multiple of anything) ->
    probabilities over 24 prompts.  'f16-resid16' = the opt-in fp16 residual stream (VG_VIT_RESID16=1, read at handle creation)."""
    from vilgod_amd.clip_wrapper import VitEncoder, clip_scores
    if dtype == 'f16-resid16':
        monkeypatch.setenv('VG_VIT_RESID16', '1')
        dtype = 'f16'
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    text = cw.synthetic_text_features(0, 24, 512)
    x = torch.randn(10, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    f_want, p_want = _oracle_probs(wd, 12, x, text)
    enc = VitEncoder(wd, dtype=dtype, device=cuda)
    f = enc.encode(x.to(cuda))
    probs, top1, score = clip_scores(f, text.to(cuda))
    f, probs, top1, score = f.cpu(), probs.cpu(), top1.cpu().numpy(), score.cpu().numpy()
    idx_want, s_want = vo.top1(p_want)
    rel = ((f - f_want).norm() / f_want.norm()).item()
    perr = (probs - p_want).abs().max().item()
    print(f'ViT-B/16 {dtype}: feature rel L2 err {rel:.2e}, max prob err {perr:.2e}')
    assert torch.allclose(probs.sum(-1), torch.ones(10), atol=1e-5)
    if dtype == 'f32':
        assert perr < TOL_PROB_F32
        assert np.array_equal(top1, idx_want)
        assert np.abs(score - s_want).max() < TOL_PROB_F32
    else:
        assert rel < 2e-2 and perr < 5e-2
        srt = np.sort(p_want.numpy(), axis=1)
        confident = (srt[:, -1] - srt[:, -2]) > 0.1
        assert np.array_equal(top1[confident], idx_want[confident])
    assert np.array_equal(top1, probs.argmax(-1).numpy())
    assert np.allclose(score, probs.max(-1).values.numpy())


@pytest.mark.gpu
def test_hip_clip_scores_exact_small(cuda):
    """D9 alone on hand-made features, incl. n = 0."""
    from vilgod_amd.clip_wrapper import clip_scores
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(33, 512, generator=g)
    text = cw.synthetic_text_features(3, 24, 512)
    want = vo.clip_probabilities(feat, text)
    probs, top1, score = clip_scores(feat.to(cuda), text.to(cuda))
    assert (probs.cpu() - want).abs().max() < 1e-5
    assert np.array_equal(top1.cpu().numpy(), vo.top1(want)[0])
    p0, t0, s0 = clip_scores(torch.zeros(0, 512, device=cuda), text.to(cuda))
    assert p0.shape == (0, 24) and t0.numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('n_crops,T', [(3, 197), (1, 50), (2, 224), (5, 33)])
def test_hip_attention_alone(cuda, n_crops, T):
    """k_attention_f16 through vg_attention against the float64 attention of the same fp16 inputs, softmax(q k^T / 8) v per (crop, head),
    model.py:175-187, under the derived per-element bound of tests/attention_ref.py (fp16 probabilities / outputs; several times tighter
    than the flat 2e-3 * max|v| this test used before), out pre-filled with NaN between guard rows."""
    import ctypes
    import attention_ref as R
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    W, H = 768, 12
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
    print(f'T={T}: worst |got - want| / bound = {worst:.3f}')


@pytest.mark.gpu
def test_hip_attention_transposing_reads_equal_transposed_image(cuda, monkeypatch):
    """T = 197: the default kernel (row-major V in LDS, V^T fragments by ds_read_b64_tr_b16) and the rounds-1-2 kernel (V written
    transposed, VG_ATT_TR=0; the switch is read per call) run the same MFMAs on the same operands: outputs bit-identical."""
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    W, H, T, n_crops = 768, 12, 197, 30
    ld = 3 * W + 64
    g = torch.Generator().manual_seed(5)
    qkv = torch.zeros(n_crops * T, ld, dtype=torch.float16)
    qkv[:, :3 * W] = (torch.randn(n_crops * T, 3 * W, generator=g) * torch.tensor([1.5] * W + [1.0] * W + [2.0] * W)).half()
    d_qkv = qkv.to(cuda)
    outs = []
    # (VG_ATT_STAGGER: the SIMD partners issue the next item's loads half a phase apart, k_attention_f16 STAG -- the same instructions
    # per wave, so the same bits; 30 crops = 360 items on 256 persistent workgroups, so the prefetch paths run)
    for tr, stag in (('1', '1'), ('1', '0'), ('0', '0')):
        monkeypatch.setenv('VG_ATT_TR', tr)
        monkeypatch.setenv('VG_ATT_STAGGER', stag)
        out = torch.zeros(n_crops * T, W, dtype=torch.float16, device=cuda)
        check(lib.vg_attention(ptr(d_qkv), ptr(out), n_crops, T, W, H, ld, stream_ptr()))
        torch.cuda.synchronize()
        outs.append(out)
    assert outs[0].abs().max().item() > 0 and all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ['patch16c1', 'patch16'])
def test_hip_vit_b16_f16_error_on_rendered_crops(cuda, rows):
    """The fp16 tower (the benchmarked mode: fp16 GEMM operands / activations, fp32 accumulate, LayerNorm and residual stream
    in fp32) against the fp32 oracle (pinned to the reference's model.py) on crops the RENDERER produced -- through the
    production path (patch rows written by the renderer, no CHW crop in between: 'patch16c1' = single-channel rows + the folded
    K = 256 patch embedding, the default; 'patch16' = three normalised channels, K = 768).  north_star's tolerance for the fp32 path is
    1e-3 on the probabilities; the fp16 mode is asserted at <= 2e-3 max probability error and <= 1e-3 relative L2 feature
    error (measured ~6e-4 / ~3.5e-4), top-1 identical wherever the oracle's margin exceeds twice that bound."""
    from vilgod_amd import synthetic
    from vilgod_amd.clip_wrapper import VitEncoder, clip_scores
    from vilgod_amd.projection import RealisticProjection
    rng = np.random.default_rng(11)
    # six object-like clusters (surface points of boxes seen from the sensor) at several ranges -> 24 crops
    clusters = []
    for k, (l, w, h) in enumerate([(4.5, 1.9, 1.6), (0.6, 0.6, 1.7), (1.8, 0.6, 1.7), (0.3, 0.3, 4.0), (8.0, 0.3, 2.5), (11.0, 2.6, 3.2)]):
        n = [900, 120, 260, 60, 1500, 2600][k]
        p = rng.uniform(-0.5, 0.5, size=(n, 3)) * [l, w, h]
        face = rng.integers(0, 2, n)
        p[face == 0, 0] = -l / 2
        p[face == 1, 1] = -w / 2
        yaw = rng.uniform(0, np.pi)
        R2 = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        p[:, :2] = p[:, :2] @ R2.T
        p += [rng.uniform(8, 45) * np.cos(k), rng.uniform(8, 45) * np.sin(k), h / 2 - 1.7]
        clusters.append(p.astype(np.float32))
    X = np.concatenate(clusters)
    seg = np.r_[0, np.cumsum([len(c) for c in clusters])].astype(np.int32)
    d_X = torch.from_numpy(X).to(cuda)
    d_index = torch.arange(len(X), dtype=torch.int32, device=cuda)
    d_seg = torch.from_numpy(seg).to(cuda)
    proj = RealisticProjection(dict(depth_bias=0.2, obj_ratio=0.8, bg_clr=0.0, resolution=112, depth=8,
                                    gaussian_kernel=dict(sigma=3, zsigma=1)), device=cuda)
    crops32 = proj.render_frame(d_X, d_index, d_seg, np.eye(4), out='f32')
    patches = proj.render_frame(d_X, d_index, d_seg, np.eye(4), out=rows)
    n = crops32.shape[0]
    assert n == 24 and float(crops32.std()) > 0.05
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    text = cw.synthetic_text_features(0, 24, 512)
    f_want, p_want = _oracle_probs(wd, 12, crops32.cpu(), text)
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    f = enc.encode_patches(patches, n)
    probs, top1, _ = clip_scores(f, text.to(cuda))
    f, probs, top1 = f.cpu(), probs.cpu(), top1.cpu().numpy()
    rel = ((f - f_want).norm() / f_want.norm()).item()
    perr = (probs - p_want).abs().max().item()
    print(f'f16 tower on {n} rendered crops ({rows}): feature rel L2 {rel:.2e}, max prob err {perr:.2e}')
    assert rel <= 1e-3 and perr <= 1e-3            # north_star's bound for the fp32 logits, met by the fp16 tower too (measured 4-6e-4)
    srt = np.sort(p_want.numpy(), axis=1)
    sure = (srt[:, -1] - srt[:, -2]) > 4e-3
    assert np.array_equal(top1[sure], vo.top1(p_want)[0][sure])


@pytest.mark.gpu
def test_hip_folded_layernorm_on_trained_like_statistics(cuda):
    """The fp16 tower folds ln_1 / ln_2 into the GEMMs around them (vit.hip k_gemm_f16_pp64 LN = 1 / 2: raw fp16 residual times
    gamma-scaled weights, row statistics applied in the epilogue).  Algebraically the same as LayerNorm followed by the GEMM
    (model.py:171-191), but the rounding differs, so it is checked where it could hurt: LayerNorm gains / offsets spread like a
    trained model's (0.3 ... 2.5, +-0.8), a few residual channels two orders of magnitude above the rest (the "massive
    activations" of trained ViTs) and a large common offset of the rows.  Reference = the fp32 tower of the same library (pinned to
    the oracle / the reference's model.py by the tests above); the folded tower must be as close to it as the tower with separate
    LayerNorm kernels (VG_VIT_LN_FOLD=0), within 1e-3 relative L2 / 2e-3 probability like the fp16 tower elsewhere."""
    from vilgod_amd.clip_wrapper import VitEncoder, clip_scores
    rng = np.random.default_rng(5)
    wd = cw.synthetic_vit_weights(3, **cw.VIT_B16)
    for k in list(wd):
        if k.endswith(('ln_1.weight', 'ln_2.weight')):
            wd[k] = torch.from_numpy(rng.uniform(0.3, 2.5, wd[k].shape).astype(np.float32))
        elif k.endswith(('ln_1.bias', 'ln_2.bias')):
            wd[k] = torch.from_numpy(rng.uniform(-0.8, 0.8, wd[k].shape).astype(np.float32))
    pos = wd['positional_embedding'].clone()
    pos[:, [7, 300, 555]] += torch.tensor([40.0, -25.0, 60.0])          # outlier channels of the residual stream
    pos += 1.5                                                          # rows with |mean| comparable to their spread
    wd['positional_embedding'] = pos
    wd['ln_pre.weight'] = torch.from_numpy(rng.uniform(0.5, 3.0, 768).astype(np.float32))
    crops = torch.from_numpy(rng.uniform(-1.8, 2.2, (12, 3, 224, 224)).astype(np.float32)).to(cuda)
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    f32 = VitEncoder(wd, dtype='f32', device=cuda).encode(crops)
    p32 = clip_scores(f32, text)[0]
    res = {}
    for fold in ('1', '0'):
        old = os.environ.get('VG_VIT_LN_FOLD')
        os.environ['VG_VIT_LN_FOLD'] = fold                              # read by vg_vit_create
        try:
            enc = VitEncoder(wd, dtype='f16', device=cuda)
        finally:
            if old is None:
                del os.environ['VG_VIT_LN_FOLD']
            else:
                os.environ['VG_VIT_LN_FOLD'] = old
        f = enc.encode(crops)
        p = clip_scores(f, text)[0]
        res[fold] = (((f - f32).norm() / f32.norm()).item(), (p - p32).abs().max().item())
        assert torch.isfinite(f).all()
    print(f'folded LayerNorm: rel L2 {res["1"][0]:.2e} / max prob err {res["1"][1]:.2e};  separate kernels: {res["0"][0]:.2e} / {res["0"][1]:.2e}')
    assert res['1'][0] <= max(1e-3, 1.5 * res['0'][0]) and res['1'][1] <= max(2e-3, 1.5 * res['0'][1])


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['w4', 'pp64'])
@pytest.mark.parametrize('width,heads', [(256, 4), (512, 8), (1024, 16)])
def test_hip_folded_layernorm_other_widths(cuda, width, heads, family, monkeypatch):
    """The consumer GEMM merges K / 128 (k_gemm_f16_w4, the default) or K / 256 (k_gemm_f16_pp64, VG_GEMM_W4=0) partial row statistics --
    2 .. 8 resp. 1 .. 4 here, 6 / 3 for ViT-B/16: the folded fp16 tower agrees with the tower that runs separate LayerNorm kernels and
    with the fp32 tower at every width the 256 x 256 kernels serve, in either kernel family."""
    from vilgod_amd.clip_wrapper import VitEncoder
    monkeypatch.setenv('VG_GEMM_W4', '1' if family == 'w4' else '0')
    rng = np.random.default_rng(width)
    wd = cw.synthetic_vit_weights(4, width=width, layers=2, heads=heads, patch=16, resolution=64, output_dim=128)
    crops = torch.from_numpy(rng.uniform(-1.8, 2.2, (40, 3, 64, 64)).astype(np.float32)).to(cuda)
    f32 = VitEncoder(wd, dtype='f32', device=cuda).encode(crops)
    res = {}
    for fold in ('1', '0'):
        old = os.environ.get('VG_VIT_LN_FOLD')
        os.environ['VG_VIT_LN_FOLD'] = fold
        try:
            enc = VitEncoder(wd, dtype='f16', device=cuda)
        finally:
            if old is None:
                del os.environ['VG_VIT_LN_FOLD']
            else:
                os.environ['VG_VIT_LN_FOLD'] = old
        f = enc.encode(crops)
        assert torch.isfinite(f).all()
        res[fold] = ((f - f32).norm() / f32.norm()).item()
    print(f'width {width}: folded {res["1"]:.2e}, separate {res["0"]:.2e} (relative L2 vs the fp32 tower)')
    assert res['1'] <= max(1e-3, 1.5 * res['0'])


@pytest.mark.gpu
@pytest.mark.parametrize('n', [3, 37, 300])
def test_hip_last_block_on_class_token_rows_only(cuda, n, monkeypatch):
    """The fp16 tower runs the last block's out_proj / MLP on the class-token rows alone (the only rows ln_post reads, model.py:235-238;
    VG_VIT_CLS_LAST=0 runs them on all n x T rows): a row's values do not depend on which rows share its GEMM tile, so the features
    are the same numbers, not merely close ones."""
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(2, **cw.VIT_B16)
    x = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).to(cuda)
    monkeypatch.setenv('VG_VIT_RESID_HL', '0')       # (the fp16-pair residual stream exists with the class-row last block only: fp32 stream on both sides)
    f_cls = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_VIT_CLS_LAST', '0')
    f_all = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    assert torch.isfinite(f_cls).all()
    assert torch.equal(f_cls, f_all), (f_cls - f_all).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [334, 340])
def test_hip_tower_with_split_k_tails(cuda, n, monkeypatch):
    """334 / 340 crops are 258 / 262 row tiles: the residual GEMMs' fourth round of tiles would hold 6 / 18 tiles on 256 CUs; the tower
    runs c_proj's share of those row tiles K-split when VG_GEMM_SPLITK=8 (opt-in: launch_gemm / splitk_plan).  The features stay within the fp16 tower's bound against the fp32 tower and
    within fp16 rounding of the unsplit run (VG_GEMM_SPLITK=0); crops whose rows lie in complete rounds only change through nothing at all
    in the first block and through attention-free row-wise work afterwards: rows never mix, so THEIR features are the same numbers."""
    monkeypatch.setenv('VG_GEMM_W4', '0')          # split-K tails exist in the k_gemm_f16_pp64 family only (read when the handle is made)
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(3, **cw.VIT_B16)
    x = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).to(cuda)
    f32 = VitEncoder(wd, dtype='f32', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_GEMM_SPLITK', '8')
    f_split = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_GEMM_SPLITK', '0')
    f_plain = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    e_split = ((f_split - f32).norm() / f32.norm()).item()
    e_plain = ((f_plain - f32).norm() / f32.norm()).item()
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows = (n * 197 + 255) // 256
    r_main = (rows * 3 // n_cu) * n_cu // 3
    first_tail_crop = r_main * 256 // 197              # crops below it have every token row in the complete rounds
    changed = (f_split != f_plain).any(dim=1)
    print(f'{n} crops: split {e_split:.2e}, unsplit {e_plain:.2e} (relative L2 vs fp32); {int(changed.sum())} crops differ, first {int(changed.nonzero()[0]) if changed.any() else -1}, '
          f'first crop with a tail row {first_tail_crop}; max |split - unsplit| {float((f_split - f_plain).abs().max()):.2e}')
    assert e_split < 1e-3 and e_split <= 1.2 * e_plain + 1e-5
    assert changed.any() and not changed[:first_tail_crop].any()
    assert ((f_split - f_plain).norm() / f_plain.norm()).item() < 5e-4

    """The gamma-scaled weights / c1 / c2 of the folded LayerNorms are derived once per handle; vg_vit_set_weight on any tensor of a
    block invalidates them, the next encode rebuilds them: a handle whose ln_2 gain and c_fc bias were replaced after its first
    encode returns bit for bit what a fresh handle with the final weights returns."""
    import ctypes
    from vilgod_amd._lib import lib, check
    from vilgod_amd.clip_wrapper import VitEncoder
    rng = np.random.default_rng(2)
    wd = cw.synthetic_vit_weights(1, **cw.VIT_B16)
    crops = torch.from_numpy(rng.uniform(-1.8, 2.2, (3, 3, 224, 224)).astype(np.float32)).to(cuda)
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    f_before = enc.encode(crops).clone()
    wd2 = dict(wd)
    for name, lo, hi in (('transformer.resblocks.4.ln_2.weight', 0.5, 2.0), ('transformer.resblocks.4.mlp.c_fc.bias', -0.5, 0.5),
                         ('transformer.resblocks.9.ln_1.bias', -0.5, 0.5)):
        wd2[name] = torch.from_numpy(rng.uniform(lo, hi, tuple(wd[name].shape)).astype(np.float32))
        t = wd2[name].contiguous()
        check(lib.vg_vit_set_weight(enc._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), 'vg_vit_set_weight')
    f_after = enc.encode(crops)
    f_fresh = VitEncoder(wd2, dtype='f16', device=cuda).encode(crops)
    assert not torch.equal(f_before, f_after)
    assert torch.equal(f_after, f_fresh)


@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_hip_captured_classification_equals_plain_launches(cuda, width):
    """BASELINE config 5's hipGraph loop: vg_vit_classify_graph (one captured graph per crop count, replayed) returns bit for bit
    what the plain launches of vg_vit_encode + vg_clip_scores return, for new crop counts (capture) and repeated ones (replay),
    on a worker stream with persistent buffers."""
    from vilgod_amd.clip_wrapper import VitEncoder, GraphClassifier, clip_scores
    wd = cw.synthetic_vit_weights(0, **cw.VIT_B16)
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    plain = enc.view()
    g = GraphClassifier(enc, text, max_crops=16, patch_width=width)       # 256: single-channel rows (level / 256), 768: normalised channels
    gen = torch.Generator().manual_seed(5)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for n in [5, 9, 5, 16, 9, 5, 20]:                     # 20 > capacity: buffers grow, graphs are rebuilt
            rows = (n * 196 + 255) // 256 * 256
            if width == 768:
                p = (torch.randn(rows, 768, generator=gen) * 0.8).half().to(cuda)
            else:
                p = (torch.randint(0, 256, (rows, 256), generator=gen).float() / 256.0).half().to(cuda)
            g.patch_buffer(n)[:rows].copy_(p)
            probs, top1, score = [t.clone() for t in g.classify(n)]
            want = clip_scores(plain.encode_patches(p, n), text)
            stream.synchronize()
            assert torch.equal(probs, want[0]) and torch.equal(top1, want[1]) and torch.equal(score, want[2]), n
    st = g.stats()
    assert st['graphs_captured'] >= 1 and st['graph_launches'] >= st['graphs_captured']



@pytest.mark.gpu
@pytest.mark.parametrize('form', ['state_dict', 'torchscript'])
def test_hip_clipwrapper_loads_a_checkpoint_end_to_end(cuda, tmp_path, form):
    """ClipWrapper's real-checkpoint path (clip_utils.py:19-26, clip.py:94-141) on the GPU with a FABRICATED checkpoint of the real
    ViT-B/16 shape: the published file is a TorchScript archive holding fp16 tensors under `visual.*` next to the text tower;
    both that form and a plain state dict must load, the cached text features next to the checkpoint must be used, and the scores
    must equal those of an encoder built directly from the same tensors.  (The real ViT-B-16.pt cannot be fetched here.)"""
    from vilgod_amd.clip_wrapper import ClipWrapper, VitEncoder, clip_scores
    from vilgod_amd.pipeline import default_preprocessor_cfg
    wd = cw.synthetic_vit_weights(5, **cw.VIT_B16)
    half = {k: v.half() for k, v in wd.items()}                          # the published checkpoint stores half tensors
    sd = {**{'visual.' + k: v for k, v in half.items()}, **{k: v.half() for k, v in cw.synthetic_text_weights(2, width=64, layers=1, embed=512).items()},
          'logit_scale': torch.tensor(4.6052)}
    ckpt = tmp_path / 'ViT-B-16.pt'
    if form == 'state_dict':
        torch.save(sd, ckpt)
    else:
        # a TorchScript archive whose state_dict carries the dotted names: a module tree with the tensors as buffers
        root = torch.nn.Module()
        for k, v in sd.items():
            parts, node = k.split('.'), root
            for p in parts[:-1]:
                if not hasattr(node, p):
                    node.add_module(p, torch.nn.Module())
                node = getattr(node, p)
            node.register_buffer(parts[-1], v)
        torch.jit.save(torch.jit.script(root), str(ckpt))
    cfg = default_preprocessor_cfg()['clip']
    text = cw.synthetic_text_features(9, len(cfg['class_list']), 512)
    np.save(str(ckpt) + '.text_features.npy', text.numpy())              # the cache ClipWrapper writes after its first run
    clip = ClipWrapper(cfg, str(tmp_path), device=cuda, dtype='f16')
    assert clip.weights_source == str(ckpt) and clip.encoder.cfg == dict(cw.VIT_B16)
    x = (torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(2)) * 1.2).half().to(cuda)
    probs, top1, score = clip.predict_probs(x)
    ref = VitEncoder({k: v.float() for k, v in half.items()}, dtype='f16', device=cuda)
    want = clip_scores(ref.encode(x), text.to(cuda))
    assert torch.equal(probs, want[0]) and torch.equal(top1, want[1])
    names, scores = clip.predict_clip_labels(x)
    assert names == [cfg['class_list'][int(i)] for i in top1.cpu()] and len(scores) == 6


@pytest.mark.gpu
def test_hip_tower_kernel_families_agree(cuda, monkeypatch):
    """The fp16 ViT-B/16 tower on k_gemm_f16_w4 (default) and on k_gemm_f16_pp64 (VG_GEMM_W4=0): the projection GEMMs themselves are
    bit-identical (tests/test_gemm.py); the folded LayerNorm's row statistics are merged from 128- resp. 256-column partials, so the
    features agree to fp32 rounding of those sums -- far inside the fp16 tower's distance to the fp32 tower."""
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(2, **cw.VIT_B16)
    x = torch.randn(40, 3, 224, 224, generator=torch.Generator().manual_seed(40)).to(cuda)
    f_w4 = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_GEMM_W4', '0')
    f_pp = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    assert torch.isfinite(f_w4).all()
    rel = ((f_w4 - f_pp).norm() / f_pp.norm()).item()
    print(f'k_gemm_f16_w4 vs k_gemm_f16_pp64 tower: relative L2 {rel:.2e}')
    assert rel < 5e-4           # (measured 1.7e-4: a last-bit difference of a row's rstd moves fp16 roundings downstream; the fp16 tower sits 3.4e-4 from the fp32 tower)


@pytest.mark.gpu
def test_hip_tower_pair_residual_stream_agrees(cuda, monkeypatch):
    """The residual stream kept as an fp16 pair (the default; VG_VIT_RESID_HL=0: fp32): hi = the copy the next GEMM reads, lo = f16(x - hi):
    22 bits of x; the residual GEMMs read and write 4 + 4 bytes per element instead of 4 + 6.  The features agree with the fp32-stream tower like the two
    kernel families agree with each other (a last-bit difference of a row statistic moves fp16 roundings downstream), both sit at the same
    distance from the fp32 tower, and the pair tower is deterministic."""
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(2, **cw.VIT_B16)
    x = torch.randn(40, 3, 224, 224, generator=torch.Generator().manual_seed(40)).to(cuda)
    f32 = VitEncoder(wd, dtype='f32', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_VIT_RESID_HL', '0')
    f_x = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    monkeypatch.setenv('VG_VIT_RESID_HL', '1')
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    f_hl = enc.encode(x).cpu()
    assert torch.isfinite(f_hl).all() and torch.equal(f_hl, enc.encode(x).cpu())
    assert not torch.equal(f_hl, f_x)                     # (the switch reached the handle)
    rel = ((f_hl - f_x).norm() / f_x.norm()).item()
    d_x, d_hl = ((f_x - f32).norm() / f32.norm()).item(), ((f_hl - f32).norm() / f32.norm()).item()
    print(f'pair stream vs fp32 stream: relative L2 {rel:.2e}; to the fp32 tower {d_hl:.2e} (fp32 stream: {d_x:.2e})')
    assert rel < 5e-4 and d_hl < 1.15 * d_x + 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize('tower,n', [('VIT_B16', 2), ('VIT_B16', 3), ('VIT_B32', 10), ('VIT_B32', 11)])
def test_hip_pair_stream_switches_on_at_its_crop_count(cuda, tower, n, monkeypatch):
    """The pair stream (`hl`) and the class-row last block (`cls_only`) both need the compact class-row buffers to fit in the qkv buffer
    (vit_plan's `cls_fits`): from 3 crops for ViT-B/16, from 11 for ViT-B/32.  Below that count both are off, so VG_VIT_RESID_HL=1
    and =0 give bit-identical features; from it on the pair stream runs: the features differ, agree within 5e-4 and keep their distance
    to the fp32 tower (as in test_hip_tower_pair_residual_stream_agrees)."""
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(5, **dict(getattr(cw, tower), layers=2))
    x = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).to(cuda)
    feats = {}
    for hl in ('1', '0'):
        monkeypatch.setenv('VG_VIT_RESID_HL', hl)
        feats[hl] = VitEncoder(wd, dtype='f16', device=cuda).encode(x).cpu()
    assert torch.isfinite(feats['1']).all()
    above = n >= {'VIT_B16': 3, 'VIT_B32': 11}[tower]
    if not above:
        assert torch.equal(feats['1'], feats['0'])
        return
    assert not torch.equal(feats['1'], feats['0'])       # (the pair stream ran)
    f32 = VitEncoder(wd, dtype='f32', device=cuda).encode(x).cpu()
    rel = ((feats['1'] - feats['0']).norm() / feats['0'].norm()).item()
    d_x, d_hl = ((feats['0'] - f32).norm() / f32.norm()).item(), ((feats['1'] - f32).norm() / f32.norm()).item()
    print(f'{tower} n = {n}: pair vs fp32 stream {rel:.2e}; to the fp32 tower {d_hl:.2e} (fp32 stream: {d_x:.2e})')
    assert rel < 5e-4 and d_hl < 1.15 * d_x + 1e-5


@pytest.mark.gpu
def test_hip_tower_is_deterministic_with_two_encodes_in_flight(cuda):
    """Race screen for k_gemm_f16_w4 under the pipeline's conditions: two encodes in flight on two streams (persistent workgroups of one
    launch start on CUs as the other launch's workgroups leave them; DMA pieces of a tile are waited for with counts that assume in-order
    retirement behind the previous tile's stores).  A fragment read that ran ahead of its piece would return stale LDS bytes without any
    fault: 2 x 12 encodes of 120 crops, every result bit-identical to the first."""
    import threading
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(1, **cw.VIT_B16)
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    n = 120
    rows = (n * 196 + 255) // 256 * 256
    g = torch.Generator().manual_seed(7)
    pats = [(torch.randint(0, 256, (rows, 256), generator=g).float() / 256).half().to(cuda) for _ in range(2)]
    views = [enc.view(), enc.view()]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    ref = []
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            ref.append(views[k].encode_patches(pats[k], n).clone())
        streams[k].synchronize()
    assert torch.isfinite(ref[0]).all() and not torch.equal(ref[0], ref[1])
    bad = []

    def loop(k):
        with torch.cuda.stream(streams[k]):
            for it in range(12):
                f = views[k].encode_patches(pats[k], n)
                streams[k].synchronize()
                if not torch.equal(f, ref[k]):
                    bad.append((k, it, (f - ref[k]).abs().max().item()))
    th = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not bad, bad


# ------------------------------------------------------------------------------- workspace layout, resolved weights
SMALL_TOWER = dict(width=256, layers=2, heads=4, patch=16, resolution=32, output_dim=64)


def _workspace_bytes_closed_form(cfg, dtype, n, fold_on):
    """vg_vit_workspace_bytes as the header has documented it since the folded LayerNorm: callers allocate by this number."""
    W, es = cfg['width'], 2 if dtype == 'f16' else 4
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1

    def pad(m):
        return (m + 255) // 256 * 256
    Mp, Pp, Kp = pad(n * T), pad(n * (T - 1)), (3 * cfg['patch'] ** 2 + 63) // 64 * 64
    b = (Mp * W * 4                     # residual stream (fp32)
         + Mp * W * es                  # LayerNorm / attention output
         + Mp * (3 * W + 256) * es      # qkv (padded row stride)
         + Mp * 4 * W * es              # hidden activations
         + Pp * Kp * es                 # patch rows
         + Pp * W * 4)                  # patch-embedding output (fp32)
    if fold_on and dtype == 'f16' and W % 256 == 0:
        b += Mp * W * 2 + Mp * (W // 64) * 8        # fp16 copy of the stream + per-row partial statistics
    return b + 1024


@pytest.mark.gpu
@pytest.mark.parametrize('fold_on', [True, False])
@pytest.mark.parametrize('tower,dtype', [('SMALL', 'f32'), ('SMALL', 'f16'), ('VIT_B16', 'f16'), ('VIT_B32', 'f16'), ('VIT_L14', 'f16')])
def test_workspace_bytes_formula(cuda, tower, dtype, fold_on, monkeypatch):
    """The workspace size is part of the ABI (callers allocate by it): it equals the closed form for every tower, with the folded
    LayerNorm on and off (VG_VIT_LN_FOLD, read when the handle is made), on both sides of every row-tile and class-row boundary."""
    import ctypes
    from vilgod_amd._lib import lib, check
    from vilgod_amd.clip_wrapper import DTYPES
    cfg = SMALL_TOWER if tower == 'SMALL' else getattr(cw, tower)
    if not fold_on:
        monkeypatch.setenv('VG_VIT_LN_FOLD', '0')
    h = ctypes.c_void_p()
    check(lib.vg_vit_create(ctypes.byref(h), cfg['width'], cfg['layers'], cfg['heads'], cfg['patch'], cfg['resolution'],
                            cfg['output_dim'], DTYPES[dtype]), 'vg_vit_create')
    try:
        got = {n: lib.vg_vit_workspace_bytes(h, n) for n in (1, 2, 3, 10, 11, 37)}
    finally:
        lib.vg_vit_destroy(h)
    assert got == {n: _workspace_bytes_closed_form(cfg, dtype, n, fold_on) for n in got}


@pytest.mark.gpu
@pytest.mark.parametrize('switches,dtype', [({}, 'f16'), ({'VG_VIT_RESID_HL': '0'}, 'f16'),
                                            ({'VG_VIT_CLS_LAST': '0', 'VG_VIT_RESID_HL': '0'}, 'f16'), ({'VG_GEMM_W4': '0'}, 'f16'),
                                            ({'VG_VIT_LN_FOLD': '0'}, 'f16'), ({'VG_VIT_RESID16': '1'}, 'f16'), ({}, 'f32')],
                         ids=['default', 'hl0', 'cls0-hl0', 'w4-0', 'fold0', 'resid16', 'f32'])
@pytest.mark.parametrize('tower', ['SMALL', 'VIT_B16'])
def test_encode_stays_inside_its_workspace(cuda, tower, switches, dtype, monkeypatch):
    """vg_vit_encode writes nothing behind the vg_vit_workspace_bytes it reports: a guard of 1 MiB behind the workspace (in the same
    allocation) keeps its byte pattern, and the features equal those from the encoder's own, generously sized workspace -- at 2 and
    3 crops, the two sides of ViT-B/16's class-row boundary, for every residual-stream form and both kernel families."""
    from vilgod_amd._lib import lib
    from vilgod_amd.clip_wrapper import VitEncoder
    for k, val in switches.items():
        monkeypatch.setenv(k, val)
    cfg = SMALL_TOWER if tower == 'SMALL' else cw.VIT_B16
    enc = VitEncoder(cw.synthetic_vit_weights(3, **cfg), dtype=dtype, device=cuda)
    guard = 1 << 20
    for n in (2, 3):
        x = torch.randn(n, 3, cfg['resolution'], cfg['resolution'], generator=torch.Generator().manual_seed(n)).to(cuda)
        enc._ws = None
        want = enc.encode(x).cpu()                                    # workspace sized for n + headroom crops
        nbytes = lib.vg_vit_workspace_bytes(enc._h, n)
        buf = torch.zeros(nbytes + guard, dtype=torch.uint8, device=cuda)
        buf[nbytes:] = 0xA5
        enc._ws, enc._ws_crops = buf, n
        got = enc.encode(x).cpu()
        torch.cuda.synchronize()
        assert enc._ws is buf
        assert bool((buf[nbytes:] == 0xA5).all()), f'{tower} n = {n}: encode wrote behind its workspace'
        assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.gpu
def test_encode_is_bit_stable_across_weight_reset(cuda):
    """Setting a block's ln_1.weight again replaces its device tensor (and, with the folded LayerNorm, the tensors derived from it):
    the same values give bit-equal features, other values give other features -- no encode keeps a pointer or a derived tensor of
    the replaced one."""
    import ctypes
    from vilgod_amd._lib import lib, check
    from vilgod_amd.clip_wrapper import VitEncoder
    wd = cw.synthetic_vit_weights(4, **SMALL_TOWER)
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(cuda)
    name = 'transformer.resblocks.1.ln_1.weight'

    def set_weight(t):
        t = t.detach().to(torch.float32).contiguous().cpu()
        with torch.cuda.device(cuda):
            check(lib.vg_vit_set_weight(enc._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), 'vg_vit_set_weight')
    f0 = enc.encode(x).cpu()
    set_weight(wd[name])
    f1 = enc.encode(x).cpu()
    assert torch.isfinite(f0).all() and torch.equal(f0, f1)
    set_weight(wd[name] * 1.5 + 0.25)
    f2 = enc.encode(x).cpu()
    assert torch.isfinite(f2).all() and not torch.equal(f2, f0)
