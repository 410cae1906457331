"""The image tower's small kernels stage by stage (csrc/vit.hip: k_im2col, k_embed_lnpre, k_layernorm, k_head, k_conv1_fold), each against
a float64 restatement under a per-element bound derived from its arithmetic (tests/vit_stages_ref.py).  No new entry point: a tower of
ZERO layers runs im2col -> patch GEMM -> k_embed_lnpre -> k_head and nothing else, a one-layer probe tower (identity in_proj, zero
out_proj / c_proj) leaves ln_1 in qkv[:, :W] and ln_2 in h, and every stage's output is read back from the caller-owned workspace,
whose layout test_vit.test_workspace_bytes_formula pins.

Which test reaches which kernel instantiation and width path (scalar: widths 128, 384, 896; vectorised: 256, 512, 768, 1024):
  test_zero_layer_stages            k_im2col<float, f16>, <f16, f16>, <float, float>, <f16, float> (K padding 588 -> 640 at every width);
                                    k_embed_lnpre<float> without the fused ln_1, both width paths, padding rows over poison;
                                    k_head<float>, out_dim 48 / 300 / 512; patch GEMM on k_gemm_f16, k_gemm_f16_pp64 (K = 192),
                                    k_gemm_f16_w4 and the fp32 kernels
  test_zero_layer_fp16_stream       k_embed_lnpre<f16> (vectorised), k_head<f16>
  test_probe_unfolded               k_layernorm<float> both paths (f32 towers 128 / 256 / 384 / 1024); k_layernorm<f16> from fp32 rows, vectorised
                                    (VG_VIT_LN_FOLD=0, 256 / 768) and scalar (384 / 896); k_layernorm<f16, f16> (VG_VIT_RESID16=1, 256)
  test_probe_fused_ln1              k_embed_lnpre<float> WITH the fused ln_1 at every width of both paths
  test_fused_ln1_equals_separate_launch   the fused ln_1 against k_layernorm<f16> bit for bit, both paths
  test_pair_stream_at_its_boundary  k_embed_lnpre<float> writing the fp16 pair (+ fused ln_1), k_head<float> on the compact class rows
  test_single_channel_fold          k_conv1_fold + vg_vit_set_input_norm (CLIP's constants and a lopsided setting), input_kind 3
  test_refold_after_set_input_norm  vit_fold_conv1's invalidation by vg_vit_set_input_norm / vg_vit_set_weight, argument checks
  test_encode_ignores_stale_workspace   every stream form on a workspace of NaN bytes and on one an encode of more crops used before

How a ratio is counted.  Every assertion is |got - want| <= bound per element.  The printed ratio leaves the output's own rounding out
on both sides, max(|err| - rounding, 0) / (bound - rounding): a correctly rounded fp32 / fp16 / pair output sits up to half a unit of
its format from the exact value, so the plain ratio of a CORRECT kernel reaches 1 and says nothing about the derived arithmetic terms
(vit_stages_ref.worst).  The float32 emulations of the CPU test stay at or below 0.5 (worst: the stream 0.13, ln_1 / ln_2 0.12, the folded
stream 0.16, and 0.43 for the folded patch embedding, where the emulation converts W1 as the source spells it, see below).

Worst ratio per stage as the GPU tests printed them on an MI355X (all far below 0.5; nothing to explain away):
  test_zero_layer_stages            pe 0.028   x 0.153   feat 0.016   chain 0.013
  test_zero_layer_fp16_stream       pe 0.003   x 0.093   feat 0.008   chain 0.062
  test_probe_unfolded   f32 towers  pe 0.025   x 0.123   ln_1 0.191   ln_2 0.191   feat 0.028
                        f16 towers  pe 0.008   x 0.140   ln_1 0.117   ln_2 0.113   feat 0.011
  test_probe_fused_ln1              pe 0.009   x 0.155   ln_1 0.126   ln_2 0.123   feat 0.013
  test_pair_stream_at_its_boundary  n = 31 (pair): pe 0.002, x 0.101, feat 0.014;   n = 30 (fp32): pe 0.002, x 0.144, feat 0.012
  test_single_channel_fold          pe 0.005   x 0.216   chain 0.004   three-channel x 0.099
                                    against the exact embedding: single-channel 0.166, three-channel 0.095; one against the other 0.083
  test_fused_ln1_equals_separate_launch, test_refold_after_set_input_norm, test_encode_ignores_stale_workspace: bit-equal, as claimed

What the tests found.  A zero-layer encode works.  The fused ln_1 IS bit-identical to the separate launch.  No stream form reads stale
workspace bytes.  One thing differs from what the source says: k_conv1_fold's W1 is spelled (f16)(float)(double), but read back through
one-hot patch rows (test_single_channel_weight_read_back) the compiled kernel holds the float64 value rounded to fp16 ONCE in every
element, also in the 5 to 9 of 65 536 where the two-step conversion lands one fp16 ulp away.  With K = 256 one such element moves a
patch-embedding dot by half of the GEMM bound, so a reference that rounds twice fails (it did: 1.5 of the bound).  Both roundings are
correct kernels; the reference rounds once and admits the difference to the two-step value (vit_stages_ref.fold_w1_slack).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import vit_stages_ref as R

CLIP_NORM = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
LOPSIDED_NORM = ((0.1, 0.5, 0.9), (0.2, 0.5, 1.5))


def _cfg(width, patch, res, out_dim):
    return dict(width=width, patch=patch, resolution=res, output_dim=out_dim)


def _case(width, patch, res, out_dim, n, dtype, kind, family, layers=0, stream=None, seed=0, probe=True, stream_scale=1.0):
    cfg = _cfg(width, patch, res, out_dim)
    crops = R.make_crops(cfg, n, seed + 1, np.float16 if kind == 1 else np.float32)
    return dict(cfg=cfg, n=n, dtype=dtype, kind=kind, stream=stream or 'f32', crops=crops,
                w=R.make_weights(cfg, family, seed, layers, probe, stream_scale))


# ------------------------------------------------------------------------------------------------------------ CPU
def test_region_restates_the_workspace_closed_form():
    from test_vit import _workspace_bytes_closed_form, SMALL_TOWER
    from vilgod_amd import clip_weights as cw
    for cfg in (SMALL_TOWER, cw.VIT_B16, cw.VIT_L14, dict(SMALL_TOWER, width=384), dict(SMALL_TOWER, patch=14, resolution=28)):
        for dtype in ('f32', 'f16'):
            for fold_on in (True, False):
                for n in (1, 2, 31, 52, 300):
                    reg = R.region(cfg, dtype, n, fold_on)
                    assert reg['total'] == _workspace_bytes_closed_form(cfg, dtype, n, fold_on)
                    names = ('x', 'h', 'qkv', 'mlp', 'patches', 'pe', 'x16', 'lnst')
                    assert sum(reg[k][1] for k in names) + 1024 == reg['total']
                    assert all(reg[a][0] + reg[a][1] == reg[b][0] for a, b in zip(names, names[1:]))
    assert R.pair_stream_from(dict(width=256, patch=16, resolution=64)) == 31          # (the test computes it; this pins the formula)
    assert R.pair_stream_from(cw.VIT_B16) == 3 and R.pair_stream_from(cw.VIT_B32) == 11   # test_vit's boundaries


CHECKER_CASES = [  # width (384: scalar path, 512: vectorised), dtype, stream, kind
    (384, 'f16', 'f32', 0), (512, 'f16', 'f32', 1), (512, 'f32', 'f32', 0), (512, 'f16', 'f16', 0), (512, 'f16', 'pair', 0)]


@pytest.mark.parametrize('family', R.FAMILIES)
def test_checker_accepts_the_emulated_kernels_and_rejects_synthesised_faults(family):
    """The checkers on float32 emulations of the kernels in their own summation order: the clean emulation passes every check with worst
    error / bound <= 0.5 on every input family, and each synthesised fault is rejected on every family -- at both width paths, for the
    fp32, fp16 and pair output, patch 14 (K padding), three crops (one of zeros: the const row is constant)."""
    worst = {}
    for width, dtype, stream, kind in CHECKER_CASES:
        case = _case(width, 14, 28, 48, 3, dtype, kind, family, layers=1, stream=stream, seed=width)
        got = R.emulate(case, layers=1)
        r = R.check_zero_layer(case, got)
        if stream != 'pair':
            r.update({k: v for k, v in R.check_probe(case, got).items() if k.startswith('ln_')})
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        faults = R.FAULTS_IM2COL + R.FAULTS_EMBED + R.FAULTS_LN + (R.FAULTS_FUSED if dtype == 'f16' and stream == 'f32' else ())
        for fault in faults:
            bad = R.emulate(case, fault, layers=1)
            with pytest.raises(AssertionError):
                R.check_zero_layer(case, bad)
                R.check_probe(case, bad)
    # ln_1, ln_2 and ln_post reject the LayerNorm faults on their own too (the stream is read as the GPU wrote it, so ln_pre's fault does not
    # help them); a missing eps shows only where a row's variance is comparable with it: the small stream (make_weights' stream_scale)
    p = 'transformer.resblocks.0.'
    for width, dtype in ((384, 'f16'), (512, 'f16'), (512, 'f32')):
        for scale in (1.0, 0.004):
            case = _case(width, 14, 28, 48, 3, dtype, 0, family, layers=1, seed=width, stream_scale=scale)
            r = R.check_probe(case, R.emulate(case, layers=1))
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            for fault in ([f for f in R.FAULTS_LN if f != 'no_eps'] if scale == 1.0 else ['no_eps']):
                bad = R.emulate(case, fault, layers=1)
                rows = R.stream_value(case, bad)[:case['n'] * 5]
                for key, ln in (('h1', 'ln_1'), ('h2', 'ln_2')):
                    with pytest.raises(AssertionError):
                        R.check_ln(rows, bad[key], case['w'][p + ln + '.weight'], case['w'][p + ln + '.bias'], dtype, key)
                with pytest.raises(AssertionError):
                    R.check_feat(case, bad)
    # the single-channel fold (patch 16 / K = 256), CLIP's constants and the lopsided setting
    for norm in (CLIP_NORM, LOPSIDED_NORM):
        cfg = _cfg(512, 16, 32, 48)
        _, rows = R.make_levels(cfg, 3, 5)
        case = dict(cfg=cfg, n=3, dtype='f16', kind=3, stream='f32', crops=rows, norm=norm, w=R.make_weights(cfg, family, 9))
        r = R.check_zero_layer(case, R.emulate(case))
        for k, v in r.items():
            worst['fold ' + k] = max(worst.get('fold ' + k, 0.0), v)
        for fault in R.FAULTS_FOLD:
            with pytest.raises(AssertionError):
                R.check_zero_layer(case, R.emulate(case, fault))
    print(f'{family}: worst error / bound of the emulations: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 0.5, worst


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
def _encoder(case, cuda):
    from vilgod_amd.clip_wrapper import VitEncoder
    enc = VitEncoder({k: torch.from_numpy(v) for k, v in case['w'].items()}, dtype=case['dtype'], device=cuda)
    if 'norm' in case:
        _set_norm(enc, case['norm'])
    return enc


def _set_norm(enc, norm):
    from vilgod_amd._lib import lib
    return lib.vg_vit_set_input_norm(enc._h, (ctypes.c_float * 3)(*norm[0]), (ctypes.c_float * 3)(*norm[1]))


def _fold_on(case):
    return case['dtype'] == 'f16' and case['cfg']['width'] % 256 == 0 and os.environ.get('VG_VIT_LN_FOLD', '1') != '0' \
        and 'VG_VIT_RESID16' not in os.environ


def _encode(enc, case, cuda, ws=None, fill=0, poison=('patches', 'pe', 'x'), crops=None, kind=None, n=None):
    """One vg_vit_encode on a caller-owned workspace (`fill` bytes everywhere, 0xA5 in the `poison` regions) -> (features, ws, regions)"""
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    n = case['n'] if n is None else n
    reg = R.region(case['cfg'], case['dtype'], n, _fold_on(case))
    nbytes = lib.vg_vit_workspace_bytes(enc._h, n)
    assert reg['total'] == nbytes, (reg['total'], nbytes)
    if ws is None:
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=cuda)
        for name in poison:
            ws[reg[name][0]:reg[name][0] + reg[name][1]] = R.POISON
    assert ws.numel() >= nbytes
    d_in = torch.from_numpy(case['crops'] if crops is None else crops).to(cuda)
    feat = torch.empty((n, case['cfg']['output_dim']), dtype=torch.float32, device=cuda)
    with torch.cuda.device(cuda):
        check(lib.vg_vit_encode(enc._h, ptr(d_in), case['kind'] if kind is None else kind, n, ptr(ws), ptr(feat), stream_ptr()), 'vg_vit_encode')
        torch.cuda.synchronize()
    return feat.cpu().numpy(), ws, reg


def _read(ws, reg, name, dtype, rows, cols, ld=None):
    off = reg[name][0]
    ld = ld or cols
    es = np.dtype(dtype).itemsize
    assert rows * ld * es <= reg[name][1] or name == 'x'
    raw = ws[off:off + rows * ld * es].cpu().numpy()
    return np.ascontiguousarray(raw.view(dtype).reshape(rows, ld)[:, :cols])


def _stages(ws, reg, case, feat, layers=0, h2=False):
    """The stages' outputs out of the workspace, in the form vit_stages_ref's checkers take."""
    W, dt = case['cfg']['width'], R.NP[case['dtype']]
    got = {'feat': feat, 'pe': _read(ws, reg, 'pe', np.float32, reg['Pp'], W)}
    if case['kind'] < 2:
        got['patches'] = _read(ws, reg, 'patches', dt, reg['Pp'], reg['Kp'])
    if case['stream'] == 'pair':
        got['lo'] = _read(ws, reg, 'x', np.float16, reg['Mp'], W)
        got['hi'] = _read(ws, reg, 'x16', np.float16, reg['Mp'], W)
    else:
        got['x'] = _read(ws, reg, 'x', np.float16 if case['stream'] == 'f16' else np.float32, reg['Mp'], W)
    if layers:
        got['h1'] = _read(ws, reg, 'qkv', dt, reg['M'], W, reg['qkv_ld'])
        if h2:
            got['h2'] = _read(ws, reg, 'h', dt, reg['M'], W)
    return got


def _say(what, r):
    print(f'{what}: worst error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in r.items()))


# ------------------------------------------------------------------------------------------------------------ 2. zero-layer towers
ZERO_LAYER = [  # width, patch, resolution, out_dim, n, dtype, input kind, family   (every width with patch 14; every value of every axis)
    (128, 14, 28, 48, 1, 'f32', 0, 'gauss'), (256, 14, 28, 300, 52, 'f16', 0, 'offset'), (384, 14, 28, 512, 1, 'f16', 1, 'massive'),
    (512, 14, 28, 48, 52, 'f32', 1, 'const'), (768, 14, 28, 300, 1, 'f16', 0, 'gauss'), (896, 14, 28, 512, 52, 'f32', 0, 'massive'),
    (1024, 14, 28, 48, 1, 'f16', 1, 'offset'), (1024, 14, 28, 512, 52, 'f16', 0, 'const'), (896, 14, 28, 300, 1, 'f16', 0, 'gauss'),
    (128, 14, 28, 300, 52, 'f16', 1, 'const'), (384, 14, 28, 48, 52, 'f32', 0, 'offset'),
    (128, 8, 16, 512, 52, 'f16', 0, 'massive'), (256, 8, 16, 48, 1, 'f32', 1, 'gauss'), (384, 8, 16, 300, 52, 'f16', 0, 'const'),
    (512, 8, 16, 512, 1, 'f16', 0, 'offset'), (768, 8, 16, 48, 52, 'f32', 0, 'gauss'), (896, 8, 16, 300, 1, 'f32', 1, 'massive'),
    (1024, 8, 16, 300, 52, 'f32', 0, 'offset'),
    (128, 16, 32, 48, 1, 'f16', 0, 'offset'), (256, 16, 32, 512, 52, 'f16', 1, 'const'), (384, 16, 32, 300, 1, 'f32', 0, 'massive'),
    (512, 16, 32, 300, 52, 'f16', 0, 'gauss'), (768, 16, 32, 512, 52, 'f16', 1, 'massive'), (896, 16, 32, 48, 52, 'f16', 0, 'offset'),
    (1024, 16, 32, 512, 1, 'f32', 0, 'gauss'),
    (128, 32, 64, 300, 1, 'f32', 0, 'gauss'), (256, 32, 64, 48, 52, 'f16', 0, 'massive'), (512, 32, 64, 512, 52, 'f32', 1, 'const'),
    (768, 32, 64, 300, 1, 'f16', 1, 'offset'), (896, 32, 64, 512, 52, 'f16', 1, 'gauss'), (1024, 32, 64, 48, 52, 'f16', 0, 'const')]


@pytest.mark.gpu
@pytest.mark.parametrize('width,patch,res,out_dim,n,dtype,kind,family', ZERO_LAYER)
def test_zero_layer_stages(cuda, width, patch, res, out_dim, n, dtype, kind, family):
    """A zero-layer tower on a workspace whose patches, pe and x regions hold 0xA5 bytes: patch rows bit-equal to im2col with zero K
    padding, patch embedding within the GEMM bound, stream within the LayerNorm bound of the float64 embedding of the GPU's own pe rows
    with its padding rows zeroed over the poison, features within the head bound of the GPU's own class rows and within the summed bound
    of the all-float64 chain."""
    case = _case(width, patch, res, out_dim, n, dtype, kind, family, seed=width + patch + n)
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    r = R.check_zero_layer(case, _stages(ws, reg, case, feat))
    _say(f'W {width} patch {patch} n {n} {dtype} kind {kind} {family}', r)


@pytest.mark.gpu
@pytest.mark.parametrize('width,family', [(256, 'offset'), (768, 'const')])
def test_zero_layer_fp16_stream(cuda, width, family, monkeypatch):
    """VG_VIT_RESID16=1: k_embed_lnpre<f16> writes fp16 rows (one fp16 rounding in the bound), k_head<f16> reads them."""
    monkeypatch.setenv('VG_VIT_RESID16', '1')
    case = _case(width, 14, 28, 300, 52, 'f16', 0, family, stream='f16', seed=width)
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    r = R.check_zero_layer(case, _stages(ws, reg, case, feat))
    _say(f'fp16 stream W {width} {family}', r)


# ------------------------------------------------------------------------------------------------------------ 3. one-layer probe towers
@pytest.mark.gpu
@pytest.mark.parametrize('dtype,width,switch,n,family,scale', [
    ('f32', 128, None, 52, 'offset', 1.0), ('f32', 256, None, 1, 'massive', 1.0), ('f32', 384, None, 52, 'const', 1.0), ('f32', 1024, None, 52, 'gauss', 1.0),
    ('f16', 256, 'VG_VIT_LN_FOLD=0', 52, 'const', 1.0), ('f16', 768, 'VG_VIT_LN_FOLD=0', 1, 'offset', 1.0), ('f16', 384, None, 1, 'gauss', 1.0),
    ('f16', 896, None, 52, 'massive', 1.0), ('f16', 256, 'VG_VIT_RESID16=1', 52, 'massive', 1.0),
    ('f32', 128, None, 52, 'gauss', 0.004), ('f32', 512, None, 52, 'offset', 0.004), ('f16', 256, 'VG_VIT_LN_FOLD=0', 52, 'massive', 0.004),
    ('f16', 384, None, 52, 'const', 0.004), ('f16', 256, 'VG_VIT_RESID16=1', 52, 'gauss', 0.004)])
def test_probe_unfolded(cuda, dtype, width, switch, n, family, scale, monkeypatch):
    """Towers that launch k_layernorm: after the encode qkv[:, :W] is ln_1 and h is ln_2 of the stream the x region still holds (different
    gains and shifts: a mix-up shows), each within the LayerNorm bound of float64 on the GPU's own rows.  scale 0.004: a stream whose rows
    have a variance comparable with the LayerNorm epsilon, the only rows on which the eps of k_layernorm and k_head shows (the CPU test
    shows that these reject a missing eps, and the rows of scale 1 every other fault)."""
    if switch:
        monkeypatch.setenv(*switch.split('='))
    stream = 'f16' if switch == 'VG_VIT_RESID16=1' else 'f32'
    case = _case(width, 8, 16, 48, n, dtype, 0, family, layers=1, stream=stream, seed=width + n, stream_scale=scale)
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    got = _stages(ws, reg, case, feat, layers=1, h2=True)
    r = R.check_probe(case, got)
    r['feat'] = R.check_feat(case, got)
    assert 'ln_2' in r
    _say(f'probe {dtype} W {width} {switch or ""} n {n} {family} scale {scale}', r)


@pytest.mark.gpu
@pytest.mark.parametrize('width,n,family,scale', [(128, 52, 'gauss', 1.0), (256, 1, 'offset', 1.0), (384, 52, 'massive', 1.0), (512, 52, 'const', 1.0),
                                                  (768, 52, 'offset', 1.0), (896, 1, 'const', 1.0), (1024, 52, 'massive', 1.0),
                                                  (384, 52, 'offset', 0.004), (512, 52, 'gauss', 0.004)])
def test_probe_fused_ln1(cuda, width, n, family, scale):
    """The default fp16 tower: ln_1 of block 0 comes out of k_embed_lnpre -- within the LayerNorm bound at every width of both paths
    (scale 0.004: on rows whose variance is comparable with eps, as in test_probe_unfolded)."""
    case = _case(width, 8, 16, 48, n, 'f16', 0, family, layers=1, seed=width + n, stream_scale=scale)
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    got = _stages(ws, reg, case, feat, layers=1, h2=width % 256 != 0)
    r = R.check_probe(case, got)
    r['feat'] = R.check_feat(case, got)
    _say(f'fused ln_1 W {width} n {n} {family} scale {scale}', r)


@pytest.mark.gpu
@pytest.mark.parametrize('width', [128, 256, 384, 768, 1024])
def test_fused_ln1_equals_separate_launch(cuda, width, monkeypatch):
    """k_embed_lnpre's comment calls its fused ln_1 "bit-identical to the separate launch": a tower whose ln_2 has ln_1's parameters, run
    unfolded, writes h by k_layernorm<f16> from the same fp32 rows -- h must equal qkv[:, :W] bit for bit."""
    monkeypatch.setenv('VG_VIT_LN_FOLD', '0')
    case = _case(width, 8, 16, 48, 52, 'f16', 0, 'massive', layers=1, seed=width)
    p = 'transformer.resblocks.0.'
    case['w'][p + 'ln_2.weight'], case['w'][p + 'ln_2.bias'] = case['w'][p + 'ln_1.weight'], case['w'][p + 'ln_1.bias']
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    got = _stages(ws, reg, case, feat, layers=1, h2=True)
    R.check_probe(case, got)
    diff = got['h1'].view(np.uint16) != got['h2'].view(np.uint16)
    assert not diff.any(), f'{int(diff.sum())} of {diff.size} elements differ between the fused ln_1 and k_layernorm<f16>'


# ------------------------------------------------------------------------------------------------------------ 4. the fp16-pair stream
PAIR_TOWER = _cfg(256, 16, 64, 64)


def _pair_case(n, stream):
    cfg = PAIR_TOWER
    return dict(cfg=cfg, n=n, dtype='f16', kind=0, stream=stream, crops=R.make_crops(cfg, n, 3), w=R.make_weights(cfg, 'massive', 4, layers=2, probe=False))


@pytest.mark.gpu
def test_pair_stream_at_its_boundary(cuda):
    """Two layers, T = 17, out_proj and c_proj zero: at the first crop count with the pair stream (computed from vit_plan's formulas) the x
    region holds lo and the x16 region hi, hi + lo within the LayerNorm + pair bound of the float64 stream from the GPU's pe, the re-split of
    block 0's two epilogues (which added 0) left hi = f16(hi + lo), and the features are the head of the hi + lo class rows; one crop fewer
    runs the fp32 stream."""
    n = R.pair_stream_from(PAIR_TOWER)
    print(f'pair stream from {n} crops')
    case = _pair_case(n, 'pair')
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda)
    assert reg['Mp'] == 768
    got = _stages(ws, reg, case, feat)
    r = {'pe': R.check_pe(case, got), 'x': R.check_stream(case, got), 'feat': R.check_feat(case, got)}
    hi, lo = got['hi'][:reg['M']], got['lo'][:reg['M']]
    assert (lo != 0).mean() > 0.5, 'the x region does not hold the lo halves: the pair stream did not run'
    resplit = (hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float16)
    assert (resplit.view(np.uint16) == hi.view(np.uint16)).all(), 'hi != f16(hi + lo)'
    _say(f'pair stream n {n}', r)
    below = _pair_case(n - 1, 'f32')
    feat, ws, reg = _encode(enc, below, cuda)
    got = _stages(ws, reg, below, feat)
    r = {'pe': R.check_pe(below, got), 'x': R.check_stream(below, got), 'feat': R.check_feat(below, got)}
    _say(f'fp32 stream n {n - 1}', r)


# ------------------------------------------------------------------------------------------------------------ 5. the single-channel fold
def _fold_case(width, patch, norm, n=3, family='gauss'):
    cfg = _cfg(width, patch, 2 * patch, 48)
    u, rows = R.make_levels(cfg, n, width + patch)
    return dict(cfg=cfg, n=n, dtype='f16', kind=3, stream='f32', crops=rows, norm=norm, w=R.make_weights(cfg, family, width + patch)), u


@pytest.mark.gpu
@pytest.mark.parametrize('norm', [CLIP_NORM, LOPSIDED_NORM], ids=['clip', 'lopsided'])
@pytest.mark.parametrize('width,patch', [(256, 16), (768, 16), (256, 32), (768, 32)])
def test_single_channel_fold(cuda, width, patch, norm):
    """input_kind 3 on a zero-layer tower: pe within the GEMM bound of rows x fp16(W1)^T with W1 from the float64 formula, the stream within
    the LayerNorm bound of the float64 embedding with pos + b1 for t > 0 and pos for t = 0; and the same tower fed CHW crops holding
    (u / 255 - mean_c) / std_c agrees with it within the two paths' summed bounds (on the stream: the class row, all a zero-layer tower's
    features read, never meets the patch embedding)."""
    case, u = _fold_case(width, patch, norm)
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda, poison=('pe', 'x'))
    got = _stages(ws, reg, case, feat)
    r = R.check_zero_layer(case, got)
    chw = dict(case, kind=0, crops=R.levels_as_crops(case['cfg'], case['n'], u, norm))
    feat0, ws0, reg0 = _encode(enc, chw, cuda)
    got0 = _stages(ws0, reg0, chw, feat0)
    r['chw x'] = R.check_stream(chw, got0)
    want, b3, b0 = R.fold_equivalence(case, chw, u)
    M = reg['M']
    r['x3 vs exact'] = R.worst(got['x'][:M], want, b3, 'single-channel stream vs the exact embedding')
    r['x0 vs exact'] = R.worst(got0['x'][:M], want, b0, 'three-channel stream vs the exact embedding')
    r['x3 vs x0'] = R.worst(got['x'][:M], got0['x'][:M], b3 + b0, 'single-channel vs three-channel stream')
    r['feat3 vs feat0'] = R.worst(feat, feat0, R.bound_head(want[::reg['T']], case['w']['ln_post.weight'], case['w']['ln_post.bias'], case['w']['proj'],
                                                          dv=(b3 + b0)[::reg['T']]), 'features of the two paths')
    _say(f'fold W {width} patch {patch}', r)


@pytest.mark.gpu
@pytest.mark.parametrize('norm', [CLIP_NORM, LOPSIDED_NORM], ids=['clip', 'lopsided'])
def test_single_channel_weight_read_back(cuda, norm):
    """One-hot patch rows (0.5 at column p of row p) make pe[p, n] = W1[n, p] / 2 exactly, so the folded weight itself is read back: every
    element is the float64 formula rounded to fp16 -- once, or through fp32 as the kernel's source spells it (the two differ in a few
    elements per 100 000, where the float sits on an fp16 tie)."""
    cfg = _cfg(256, 16, 32, 48)
    rows = np.zeros((256, 256), np.float16)
    rows[np.arange(256), np.arange(256)] = 0.5
    case = dict(cfg=cfg, n=64, dtype='f16', kind=3, stream='f32', crops=rows, norm=norm, w=R.make_weights(cfg, 'gauss', 272))
    enc = _encoder(case, cuda)
    feat, ws, reg = _encode(enc, case, cuda, poison=('pe', 'x'))
    W1 = 2.0 * _read(ws, reg, 'pe', np.float32, 256, 256).astype(np.float64).T
    x = R.fold_w1_exact(case['w']['conv1.weight'], norm[1])
    once, twice = x.astype(np.float16).astype(np.float64), R.f16r(x)
    assert ((W1 == once) | (W1 == twice)).all(), f'{int(((W1 != once) & (W1 != twice)).sum())} elements of W1 are neither rounding of the formula'
    print(f'W1: {int((once != twice).sum())} of {W1.size} elements differ between the roundings; the kernel holds the once-rounded value in '
          f'{int(((W1 == once) & (once != twice)).sum())} of them')


@pytest.mark.gpu
def test_refold_after_set_input_norm(cuda):
    """vg_vit_set_input_norm and vg_vit_set_weight('positional_embedding') after an encode invalidate the folded tensors: the next encode
    equals a fresh handle's bit for bit (stream and features); a std <= 0 or a null pointer is VG_ERR_ARG and leaves the handle as it was."""
    from vilgod_amd._lib import lib, check
    case, _ = _fold_case(256, 16, CLIP_NORM, family='offset')

    def run(enc, c):
        feat, ws, reg = _encode(enc, c, cuda, poison=('pe', 'x'))
        return feat, _read(ws, reg, 'x', np.float32, reg['Mp'], c['cfg']['width'])
    enc = _encoder(case, cuda)
    f_clip, x_clip = run(enc, case)
    assert _set_norm(enc, LOPSIDED_NORM) == 0
    other = dict(case, norm=LOPSIDED_NORM)
    f_lop, x_lop = run(enc, other)
    f_fresh, x_fresh = run(_encoder(other, cuda), other)
    assert not np.array_equal(x_lop, x_clip)
    assert np.array_equal(x_lop.view(np.uint32), x_fresh.view(np.uint32)) and np.array_equal(f_lop.view(np.uint32), f_fresh.view(np.uint32))
    pos = np.ascontiguousarray(case['w']['positional_embedding'][::-1] * np.float32(0.75))
    with torch.cuda.device(cuda):
        check(lib.vg_vit_set_weight(enc._h, b'positional_embedding', ctypes.c_void_p(pos.ctypes.data), pos.size), 'vg_vit_set_weight')
    moved = dict(other, w=dict(case['w'], positional_embedding=pos))
    f_pos, x_pos = run(enc, moved)
    f_fresh, x_fresh = run(_encoder(moved, cuda), moved)
    assert not np.array_equal(x_pos, x_lop)
    assert np.array_equal(x_pos.view(np.uint32), x_fresh.view(np.uint32)) and np.array_equal(f_pos.view(np.uint32), f_fresh.view(np.uint32))
    R.check_stream(moved, dict(x=x_pos, pe=_read(*_encode(enc, moved, cuda, poison=('pe', 'x'))[1:], 'pe', np.float32, 256, 256)))
    three = ctypes.c_float * 3
    assert lib.vg_vit_set_input_norm(enc._h, three(0.1, 0.2, 0.3), three(1.0, 0.0, 1.0)) == 1
    assert lib.vg_vit_set_input_norm(enc._h, three(0.1, 0.2, 0.3), three(1.0, 1.0, -2.0)) == 1
    assert lib.vg_vit_set_input_norm(enc._h, None, three(1.0, 1.0, 1.0)) == 1
    assert lib.vg_vit_set_input_norm(enc._h, three(0.1, 0.2, 0.3), None) == 1
    assert lib.vg_vit_set_input_norm(None, three(0.1, 0.2, 0.3), three(1.0, 1.0, 1.0)) == 1
    f_again, x_again = run(enc, moved)
    assert np.array_equal(x_again.view(np.uint32), x_pos.view(np.uint32)) and np.array_equal(f_again.view(np.uint32), f_pos.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 6. stale workspaces
STREAM_FORMS = [({}, 'f16'), ({'VG_VIT_RESID_HL': '0'}, 'f16'), ({'VG_VIT_CLS_LAST': '0', 'VG_VIT_RESID_HL': '0'}, 'f16'), ({'VG_GEMM_W4': '0'}, 'f16'),
                ({'VG_VIT_LN_FOLD': '0'}, 'f16'), ({'VG_VIT_RESID16': '1'}, 'f16'), ({}, 'f32'), ({}, 'pair')]


@pytest.mark.gpu
@pytest.mark.parametrize('switches,dtype', STREAM_FORMS, ids=['default', 'hl0', 'cls0-hl0', 'w4-0', 'fold0', 'resid16', 'f32', 'pair-boundary'])
def test_encode_ignores_stale_workspace(cuda, switches, dtype, monkeypatch):
    """Production reuses one workspace across crop counts, so the carve-up moves over stale data: the features do not depend on what the
    workspace held -- zeros, 0xFF bytes (NaN in both types), or the leftovers of an encode of more crops."""
    from test_vit import SMALL_TOWER
    from vilgod_amd import clip_weights as cw
    for k, val in switches.items():
        monkeypatch.setenv(k, val)
    if dtype == 'pair':
        n = R.pair_stream_from(PAIR_TOWER)
        case = _pair_case(n, 'pair')
        case['w'] = {k: v.numpy() for k, v in cw.synthetic_vit_weights(3, **dict(PAIR_TOWER, layers=2, heads=4)).items()}
        many, few = n, n - 1                   # (the pair stream, then the fp32 stream over its leftovers)
    else:
        cfg = {k: SMALL_TOWER[k] for k in ('width', 'patch', 'resolution', 'output_dim')}
        wd = cw.synthetic_vit_weights(3, **SMALL_TOWER)
        case = dict(cfg=cfg, n=5, dtype=dtype, kind=0, stream='f32', w={k: v.numpy() for k, v in wd.items()})
        many, few = 5, 2
    rng = np.random.default_rng(6)
    res = case['cfg']['resolution']
    crops = rng.standard_normal((many, 3, res, res)).astype(np.float32)
    enc = _encoder(case, cuda)
    f_zero, _, _ = _encode(enc, case, cuda, poison=(), crops=crops, n=many)
    f_nan, ws, _ = _encode(enc, case, cuda, fill=0xFF, poison=(), crops=crops, n=many)
    assert np.isfinite(f_zero).all() and np.isfinite(f_nan).all()
    assert np.array_equal(f_zero.view(np.uint32), f_nan.view(np.uint32)), 'features depend on what the workspace held (NaN bytes)'
    f_few_fresh, _, _ = _encode(enc, case, cuda, poison=(), crops=crops[:few].copy(), n=few)
    f_few_reused, _, _ = _encode(enc, case, cuda, ws=ws, crops=crops[:few].copy(), n=few)
    assert np.isfinite(f_few_reused).all()
    assert np.array_equal(f_few_fresh.view(np.uint32), f_few_reused.view(np.uint32)), 'features depend on the previous encode in the same workspace'
