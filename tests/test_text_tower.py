"""The CLIP text tower on the device (include/vilgod_hip.h vg_text_*, vg_attention_causal_rows; csrc/vit_text.inc, the CAUSAL forms of
k_attention_f16 / k_attention_f32) and its Python side (clip_text.TextTower, ClipWrapper(text='device')).

Fixture: tests/golden/text_tower_golden.npz, the REFERENCE's CLIP.encode_text on a seeded two-head tower and hand-made token rows
(tests/golden/make_text_tower.py).  References: tests/text_tower_ref.py (the model in float64, the float64 masked attention) and the
per-element attention bounds of tests/attention_ref.py, whose T term stays valid because a row sees at most T keys.

CPU: the host path and the float64 restatement against the fixture, the host path's own error e_host against float64 (printed), the
refusals and the configuration plumbing.  GPU, kernel level (A-E): the causal attention against float64, row i bit-identical to the plain
kernel on the first i + 1 tokens, independence from everything behind a row, the persistent loop, the refusals.  GPU, tower level (F-J):
vg_text_encode against the fixture and float64 (e_dev <= 8 e_host, both measured and printed), fp16 against fp32 (relative L2 <= 1e-3),
bitwise independence from padding, batch companions, chunking and handle history, clamping, and ClipWrapper(text='device').
Run with -s for the figures."""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import attention_ref as R
import text_tower_ref as TR
from conftest import ROOT
from vilgod_amd import clip_text, clip_weights as cw

VG_OK, VG_ERR_ARG = 0, 1
BAR = 2e-5                 # tests/test_text.py's bar for the host path against the reference
S = 1.0                    # safety factor of the attention bounds


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'text_tower_golden.npz'))


@functools.lru_cache(maxsize=2)
def _weights(width, layers, embed, seed=0):
    return cw.synthetic_text_weights(seed, width=width, layers=layers, embed=embed)


@functools.lru_cache(maxsize=None)
def _case(width, layers, embed, dirty=True):
    """(tokens, host features float64, float64 features, e_host) of one tower on the fixture's kind of token rows: computed once, shared"""
    tokens = TR.make_tokens(TR.EOT_POSITIONS, seed=20, dirty_rows=(20,) if dirty else ())
    sd = _weights(width, layers, embed)
    host = clip_text.encode_text(sd, tokens).double()
    f64 = TR.encode_text_f64(sd, tokens)
    return tokens, host, f64, float((host - f64).abs().max())


# ===================================================================================================================== CPU
def test_fixture_rows_are_what_the_generator_describes(gold):
    tok = gold['tokens']
    assert tok.shape == (13, 77) and (tok[:, 0] == TR.SOT).all() and tok.max() == TR.EOT
    assert tuple(tok.argmax(1)[:12]) == TR.EOT_POSITIONS and tok.argmax(1)[12] == 20
    assert all((tok[r, e + 1:] == 0).all() for r, e in enumerate(TR.EOT_POSITIONS)) and (tok[12, 21:] > 0).all()
    assert np.array_equal(tok, TR.make_tokens(TR.EOT_POSITIONS, seed=20, dirty_rows=(20,)))
    assert (int(gold['width']), int(gold['layers']), int(gold['heads']), int(gold['embed'])) == (128, 2, 2, 64)


def test_host_tower_matches_reference_at_two_heads(gold):
    sd = _weights(128, 2, 64)
    f = clip_text.encode_text(sd, gold['tokens']).numpy()
    err = np.abs(f - gold['features']).max()
    print(f'host encode_text vs the reference fixture (width 128, 2 heads): {err:.2e}')
    assert f.shape == gold['features'].shape and err <= BAR


def test_float64_restatement_matches_reference(gold):
    err = np.abs(TR.encode_text_f64(_weights(128, 2, 64), gold['tokens']).numpy() - gold['features']).max()
    print(f'encode_text_f64 vs the reference fixture: {err:.2e}')
    assert err <= BAR


@pytest.mark.parametrize('width,layers,embed', [(128, 2, 64), (256, 2, 64)])
def test_host_error_against_float64(width, layers, embed):
    tokens, host, f64, e_host = _case(width, layers, embed)
    print(f'e_host (width {width}, {layers} layers): {e_host:.2e} on features of magnitude <= {float(f64.abs().max()):.2f}')
    assert 0 < e_host <= BAR


def test_host_tower_ignores_tokens_behind_eot():
    """what follows eot changes nothing, exactly: the causal mask keeps it out of every row up to eot"""
    sd = _weights(128, 2, 64)
    clean = TR.make_tokens(TR.EOT_POSITIONS, seed=20)
    dirty = clean.copy()
    g = np.random.default_rng(5)
    for r, e in enumerate(TR.EOT_POSITIONS):
        dirty[r, e + 1:] = g.integers(1, TR.SOT, 76 - e)
    assert torch.equal(clip_text.encode_text(sd, clean), clip_text.encode_text(sd, dirty))


def test_text_mode_is_refused_and_plumbed_without_a_gpu(monkeypatch):
    from vilgod_amd.clip_wrapper import ClipWrapper
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    from vilgod_amd import zero_shot_detector as zsd
    clip = default_preprocessor_cfg()['clip']
    for bad in ('gpu', 'Device', ''):
        with pytest.raises(ValueError):
            ClipWrapper(clip, '/nonexistent', device='cpu', text=bad)
    with pytest.raises(ValueError):
        ClipWrapper(clip, '/nonexistent', device='cpu', text='device', text_dtype='bf16')
    with pytest.raises(ValueError):
        clip_text.text_features('/nonexistent', ['a'], tower='gpu')
    sig = inspect.signature(PseudoLabelPipeline.__init__).parameters
    assert sig['text'].default == 'host' and sig['text_dtype'].default == 'f32'
    sig = inspect.signature(ClipWrapper.__init__).parameters
    assert sig['text'].default == 'host' and sig['text_dtype'].default == 'f32'
    text = open(os.path.join(ROOT, 'tools', 'configs', 'preprocessing.yaml')).read()
    assert re.search(r'^\s+text:\s*host\b', text, flags=re.M) and re.search(r'^\s+text_dtype:\s*f32\b', text, flags=re.M)
    for rel in ('tools/preprocess_data.py', 'vilgod_amd/zero_shot_detector.py'):
        src = open(os.path.join(ROOT, rel)).read()
        assert "text=dev.get('text', 'host')" in src and "text_dtype=dev.get('text_dtype', 'f32')" in src, rel

    # device.text = device reaches PseudoLabelPipeline through the stage dispatcher
    class Stop(Exception):
        pass
    seen = {}

    def recorder(*a, **kw):
        seen.update(kw)
        raise Stop()

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    cfg = Cfg(device={'text': 'device', 'text_dtype': 'f16'}, pipeline=[], preprocessor=None, paths=Cfg(clip_model='/nonexistent'))
    ds = Cfg(sequence_length=1)
    monkeypatch.setattr(zsd, 'PseudoLabelPipeline', recorder)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    with pytest.raises(Stop):
        zsd.ZeroShotDetector(ds, 'seq', cfg, None)
    assert seen['text'] == 'device' and seen['text_dtype'] == 'f16' and seen['pack'] == 'host'


def test_causal_kernels_are_built_without_scratch():
    from vilgod_amd import build
    asm = build._device_asm('vit.hip')
    causal = re.findall(r'^(_Z15k_attention_f16ILb0ELi(\d)ELi0ELb0ELb0ELb1E\S*):', asm, flags=re.M)
    assert sorted(int(n) for _, n in causal) == [1, 2, 3, 4, 5, 6, 7]
    assert re.search(r'^_Z15k_attention_f32ILb1E\S*:', asm, flags=re.M) and re.search(r'^_Z12k_text_embed\S*:', asm, flags=re.M)
    assert build.check_scratch('vit.hip', 'k_attention') == [] and build.check_scratch('vit.hip', 'k_text_embed') == []


# ===================================================================================================================== GPU, kernel level
def _causal(dtype, d_qkv, buf, n, T, W, H, ld, row_offset=0):
    """vg_attention_causal_rows into the rows between the guard rows of `buf` (or at `row_offset` rows behind them)."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    out = None if buf is None else ctypes.c_void_p(buf.data_ptr() + (1 + row_offset) * W * buf.element_size())
    return lib.vg_attention_causal_rows(dtype, ptr(d_qkv), out, n, T, W, H, ld, stream_ptr())


def _plain(dtype, d_qkv, buf, n, T, W, H, ld):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    out = ctypes.c_void_p(buf.data_ptr() + W * buf.element_size())
    return lib.vg_attention_rows(dtype, ptr(d_qkv), out, n, T, W, H, ld, R.n_tiles(T), stream_ptr())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _qkv(family, n, T, W, H, f32, seed=0):
    """inputs with NaN padding columns (dtype 1: ld = 3 W + 64) and 32 NaN rows behind the last item"""
    ld = 3 * W if f32 else 3 * W + 64
    qkv, _ = R.make_qkv(family, n, T, W, H, ld, 1000 * T + W + seed + (7 if f32 else 0), torch.float32 if f32 else torch.float16)
    return torch.cat([qkv, torch.full((32, ld), float('nan'), dtype=qkv.dtype)]), ld


A_CASES = [(1, T, 128, 2) for T in (1, 2, 31, 32, 33, 63, 64, 65, 77, 96, 97, 197, 224)] + [(1, 77, 768, 12)] + \
          [(0, T, 128, 2) for T in (1, 2, 63, 64, 65, 77, 128, 129, 282)] + [(0, 77, 768, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gauss', 'hot'])
@pytest.mark.parametrize('dtype,T,W,H', A_CASES)
def test_causal_attention_against_float64(cuda, dtype, T, W, H, family):
    """A: every NKB instantiation at its first and last token count, the diagonal block with 1 .. 32 rows, both dtypes, Gaussian logits
    and logits to +-100, under attention_ref's per-element bounds; guard rows untouched, every computed element finite."""
    n, f32 = 2, dtype == 0
    qkv, ld = _qkv(family, n, T, W, H, f32)
    want, A = TR.causal_reference(qkv[:n * T], n, T, W, H)
    bnd = (R.bound_f32 if f32 else R.bound_f16)(qkv[:n * T], n, T, W, H, want, A, S)
    buf = R.guarded_out(n * T, W, qkv.dtype, cuda)
    assert _causal(dtype, qkv.to(cuda), buf, n, T, W, H, ld) == VG_OK
    torch.cuda.synchronize()
    worst = R.check(buf, want, bnd, n, T, None, f'causal dtype {dtype} {family} T={T} W={W}')
    print(f'causal dtype {dtype} {family} {n}x{T} W={W}: worst |got - want| / bound = {worst:.3f}')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [1, 0])
def test_causal_row_equals_plain_kernel_on_its_prefix(cuda, dtype):
    """B: row i of the causal output == row i of vg_attention_rows (non-causal) on the item's first i + 1 tokens, bit for bit: masked
    terms enter as exact zeros, the visible ones are summed in the same order.  Catches a wrong diagonal mask, a skipped visible block
    and an off-by-one in the block skip."""
    n, T, W, H, f32 = 3, 77, 128, 2, dtype == 0
    for family in ('gauss', 'hot'):
        qkv, ld = _qkv(family, n, T, W, H, f32, seed=3)
        buf = R.guarded_out(n * T, W, qkv.dtype, cuda)
        assert _causal(dtype, qkv.to(cuda), buf, n, T, W, H, ld) == VG_OK
        torch.cuda.synchronize()
        got = buf[1:-1].cpu().reshape(n, T, W)
        assert bool(torch.isfinite(got).all())
        for i in (0, 1, 31, 32, 33, 63, 64, 76):
            Tp = i + 1
            pre = qkv[:n * T].reshape(n, T, ld)[:, :Tp].reshape(n * Tp, ld).contiguous()
            pbuf = R.guarded_out(n * Tp, W, qkv.dtype, cuda)
            assert _plain(dtype, pre.to(cuda), pbuf, n, Tp, W, H, ld) == VG_OK
            torch.cuda.synchronize()
            want = pbuf[1:-1].cpu().reshape(n, Tp, W)[:, i]
            assert torch.equal(_bits(got[:, i].contiguous()), _bits(want.contiguous())), (family, i)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [1, 0])
def test_causal_rows_do_not_depend_on_what_follows(cuda, dtype):
    """C: q, k and v rows r .. T - 1 overwritten with large finite values (+-6e4 in fp16, +-1e30 in fp32) leave output rows below r
    bit-identical to the run with zeros there; NaN in the rows behind the last item and in the padding columns reaches nothing; the
    guard rows around out are untouched."""
    n, T, W, H, f32 = 2, 77, 128, 2, dtype == 0
    big = 1e30 if f32 else 6e4
    base, ld = _qkv('gauss', n, T, W, H, f32, seed=9)
    sign = torch.where(torch.rand(T, 3 * W, generator=torch.Generator().manual_seed(1)) < 0.5, -1.0, 1.0)
    for r in (1, 32, 33, 64):
        outs = []
        for fill in (0.0, big):
            qkv = base.clone()
            v = qkv[:n * T].reshape(n, T, ld)
            v[:, r:, :3 * W] = (sign[r:] * fill).to(qkv.dtype)
            buf = R.guarded_out(n * T, W, qkv.dtype, cuda)
            assert _causal(dtype, qkv.to(cuda), buf, n, T, W, H, ld) == VG_OK
            torch.cuda.synchronize()
            buf = buf.cpu()
            assert bool((buf[0] == R.GUARD).all()) and bool((buf[-1] == R.GUARD).all())
            outs.append(buf[1:-1].reshape(n, T, W)[:, :r].contiguous())
        assert bool(torch.isfinite(outs[0]).all())
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), r


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [1, 0])
def test_causal_persistent_loop(cuda, dtype):
    """D: 300 prompts x 2 heads = 600 items at T = 77, more items than persistent workgroups: every prompt's rows equal those of a
    launch that holds this prompt alone (one item per workgroup, no prefetch of a next item), bit for bit."""
    n, T, W, H, f32 = 300, 77, 128, 2, dtype == 0
    qkv, ld = _qkv(['gauss', 'hot', 'sink'] * 100, n, T, W, H, f32, seed=4)
    d_qkv = qkv.to(cuda)
    full = R.guarded_out(n * T, W, qkv.dtype, cuda)
    assert _causal(dtype, d_qkv, full, n, T, W, H, ld) == VG_OK
    single = R.guarded_out(n * T, W, qkv.dtype, cuda)
    for c in range(n):
        assert _causal(dtype, d_qkv[c * T:], single, 1, T, W, H, ld, row_offset=c * T) == VG_OK
    torch.cuda.synchronize()
    full, single = full.cpu(), single.cpu()
    assert bool(torch.isfinite(full[1:-1]).all()) and bool((full[-1] == R.GUARD).all())
    assert torch.equal(_bits(full), _bits(single))


@pytest.mark.gpu
def test_causal_refusals(cuda):
    """E: VG_ERR_ARG and nothing launched"""
    W, H = 128, 2
    z16 = torch.zeros(300 * 2, 3 * W + 64, dtype=torch.float16, device=cuda)
    z32 = torch.zeros(300 * 2, 3 * W, dtype=torch.float32, device=cuda)
    b16, b32 = R.guarded_out(600, W, torch.float16, cuda), R.guarded_out(600, W, torch.float32, cuda)
    bad = [(1, z16, b16, 2, 225, W, H, 3 * W + 64), (0, z32, b32, 2, 283, W, H, 3 * W), (0, z32, b32, 2, 77, W, H, 3 * W + 64),
           (1, z16, b16, 2, 77, W, 3, 3 * W + 64), (0, z32, b32, 2, 77, W, 1, 3 * W), (1, None, b16, 2, 77, W, H, 3 * W + 64),
           (1, z16, None, 2, 77, W, H, 3 * W + 64), (0, None, b32, 2, 77, W, H, 3 * W), (2, z16, b16, 2, 77, W, H, 3 * W + 64),
           (1, z16, b16, 0, 77, W, H, 3 * W + 64), (1, z16, b16, 2, 0, W, H, 3 * W + 64)]
    for a in bad:
        assert _causal(*a) == VG_ERR_ARG, a[:1] + a[3:]
    torch.cuda.synchronize()
    assert bool(torch.isnan(b16[1:-1]).all()) and bool(torch.isnan(b32[1:-1]).all())
    assert _causal(1, z16, b16, 2, 224, W, H, 3 * W + 64) == VG_OK and _causal(0, z32, b32, 2, 282, W, H, 3 * W) == VG_OK
    torch.cuda.synchronize()


# ===================================================================================================================== GPU, tower level
def _tower(width, layers, embed, dtype, cuda):
    return clip_text.TextTower(_weights(width, layers, embed), dtype=dtype, device=cuda)


def _encode(width, layers, embed, dtype, cuda, tokens):
    t = _tower(width, layers, embed, dtype, cuda)
    try:
        f = t.encode(tokens)
        torch.cuda.synchronize()
        return f.cpu()
    finally:
        t.close()


@pytest.mark.gpu
def test_device_f32_tower_matches_reference_fixture(cuda, gold):
    """F: dtype 0 on the fixture's tower and tokens against the reference's features: the host path's bar"""
    f = _encode(128, 2, 64, 'f32', cuda, gold['tokens']).numpy()
    err = np.abs(f - gold['features']).max()
    print(f'device f32 tower vs the reference fixture: {err:.2e}')
    assert f.shape == gold['features'].shape and err <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize('width,layers,embed', [(128, 2, 64), (256, 2, 64), (512, 12, 512), (768, 12, 768)])
def test_device_f32_tower_against_float64(cuda, width, layers, embed):
    """F: e_dev <= 8 e_host against the float64 model, both measured here on the same case.  The margin covers another summation order
    (k_gemm_f32_mfma's K split, the attention's chains); a dropped or doubled term moves a feature by 1e-3 or more."""
    tokens, host, f64, e_host = _case(width, layers, embed, width <= 256)
    dev = _encode(width, layers, embed, 'f32', cuda, tokens).double()
    e_dev = float((dev - f64).abs().max())
    print(f'width {width}, {layers} layers: e_dev {e_dev:.2e}, e_host {e_host:.2e}, ratio {e_dev / e_host:.2f} (features <= {float(f64.abs().max()):.2f})')
    assert bool(torch.isfinite(dev).all()) and e_dev <= 8 * e_host


@pytest.mark.gpu
@pytest.mark.parametrize('width,layers,embed', [(128, 2, 64), (256, 2, 64), (512, 12, 512)])
def test_device_f16_tower_against_f32_tower(cuda, width, layers, embed):
    """G: dtype 1 (width 128: separate LayerNorms; 256 and 512: folded) against the dtype-0 device tower: relative L2 per normalised
    row <= 1e-3, the image tower's fp16 bar in tests/test_vit.py."""
    tokens = _case(width, layers, embed, width <= 256)[0]
    a = _encode(width, layers, embed, 'f32', cuda, tokens).double()
    b = _encode(width, layers, embed, 'f16', cuda, tokens).double()
    a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    rel = float((a - b).norm(dim=-1).max())
    print(f'width {width}, {layers} layers: f16 vs f32 tower, worst relative L2 of a normalised row {rel:.2e}')
    assert bool(torch.isfinite(b).all()) and rel <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('width,dtype', [(128, 'f32'), (128, 'f16'), (256, 'f16')])
def test_device_tower_rows_are_independent(cuda, width, dtype):
    """H: bit for bit -- tokens behind eot, batch companions (1, 3, 4, 131 prompts holding the same rows), TextTower's chunks against
    one vg_text_encode of all 300 prompts, and two encodes on one handle against two fresh handles."""
    clean = TR.make_tokens(TR.EOT_POSITIONS, seed=20)
    dirty = clean.copy()
    g = np.random.default_rng(5)
    for r, e in enumerate(TR.EOT_POSITIONS):
        dirty[r, e + 1:] = g.integers(1, TR.SOT, 76 - e)
    big = np.concatenate([dirty, clean] * 12)[:300]                  # 300 prompts: two chunks of TextTower.encode
    t = _tower(width, 2, 64, dtype, cuda)
    try:
        base = t.encode(clean).cpu()
        assert bool(torch.isfinite(base).all())
        assert torch.equal(_bits(t.encode(dirty).cpu()), _bits(base)), 'tokens behind eot'
        for n in (1, 3, 4, 131):
            rows = np.arange(n) % len(clean)
            assert torch.equal(_bits(t.encode(clean[rows]).cpu()), _bits(base[rows])), f'{n} prompts'
        chunked = t.encode(big).cpu()
        tok = torch.from_numpy(big).to(torch.int32).to(cuda)
        eot = TR.eot_of(big).to(torch.int32).to(cuda)
        assert torch.equal(_bits(chunked), _bits(t.encode_chunk(tok, eot).cpu())), 'chunks of 256 vs one encode of 300'
        second = t.encode(clean).cpu()
    finally:
        t.close()
    assert torch.equal(_bits(second), _bits(base))
    for _ in range(2):
        assert torch.equal(_bits(_encode(width, 2, 64, dtype, cuda, clean)), _bits(base)), 'fresh handle'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_device_tower_clamps_eot_and_token_ids(cuda, dtype):
    """I: an eot of -1 or 77 and a token id of 49408 (or negative) are clamped on the device: VG_OK, finite output, the clamped row"""
    clean = TR.make_tokens(TR.EOT_POSITIONS, seed=20)[:4]
    t = _tower(128, 2, 64, dtype, cuda)
    try:
        tok = torch.from_numpy(clean).to(torch.int32).to(cuda)
        want = t.encode_chunk(tok, torch.tensor([0, 76, 0, 76], dtype=torch.int32, device=cuda)).cpu()
        got = t.encode_chunk(tok, torch.tensor([-1, 77, -(2 ** 31), 2 ** 31 - 1], dtype=torch.int32, device=cuda)).cpu()
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want))
        bad = tok.clone()
        bad[0, 1], bad[1, 0], bad[2, 5] = 49408, -3, 2 ** 31 - 1
        ok = tok.clone()
        ok[0, 1], ok[1, 0], ok[2, 5] = 49407, 0, 49407
        eot = TR.eot_of(clean).to(torch.int32).to(cuda)
        got, want = t.encode_chunk(bad, eot).cpu(), t.encode_chunk(ok, eot).cpu()
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want))
    finally:
        t.close()


@pytest.mark.gpu
def test_device_tower_refuses_what_it_cannot_run(cuda):
    from vilgod_amd._lib import lib
    h = ctypes.c_void_p()
    for args in ((192, 2, 3, 77, 49408, 64, 0), (128, 2, 3, 77, 49408, 64, 0), (128, 2, 2, 225, 49408, 64, 1), (128, 2, 2, 0, 49408, 64, 0),
                 (2048, 2, 32, 77, 49408, 64, 1), (128, 2, 2, 77, 49408, 64, 2), (128, 2, 2, 77, 0, 64, 0)):
        assert lib.vg_text_create(ctypes.byref(h), *args) == VG_ERR_ARG, args
    assert lib.vg_text_create(ctypes.byref(h), 128, 1, 2, 77, 100, 64, 0) == VG_OK
    try:
        w = torch.zeros(100 * 128)
        assert lib.vg_text_set_weight(h, b'token_embedding.weight', ctypes.c_void_p(w.data_ptr()), 99 * 128) == VG_ERR_ARG
        assert lib.vg_text_set_weight(h, b'positional_embedding', ctypes.c_void_p(w.data_ptr()), 76 * 128) == VG_ERR_ARG
        assert lib.vg_text_set_weight(h, b'token_embedding.weight', ctypes.c_void_p(w.data_ptr()), 100 * 128) == VG_OK
        assert lib.vg_text_workspace_bytes(h, 12) > 0 and lib.vg_text_workspace_bytes(h, 0) == 0
        ws = torch.zeros(int(lib.vg_text_workspace_bytes(h, 1)), dtype=torch.uint8, device=cuda)
        tok, eot = torch.zeros(77, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
        feat = torch.zeros(64, device=cuda)
        from vilgod_amd._lib import ptr, stream_ptr
        assert lib.vg_text_encode(h, ptr(tok), ptr(eot), 1, ptr(ws), ptr(feat), stream_ptr()) == VG_ERR_ARG      # weights missing
        assert lib.vg_text_encode(h, None, ptr(eot), 1, ptr(ws), ptr(feat), stream_ptr()) == VG_ERR_ARG
    finally:
        lib.vg_text_destroy(h)


class _WordTokenizer:
    """stand-in for the BPE tokenizer: every word a fixed id, so that no merges file is needed"""

    @staticmethod
    def tokenize_prompts(prompts, bpe_path=None):
        import zlib
        out = np.zeros((len(prompts), 77), np.int64)
        for i, p in enumerate(prompts):
            ids = [TR.SOT] + [1 + zlib.crc32(w.encode()) % 49000 for w in p.lower().split()] + [TR.EOT]
            out[i, :len(ids)] = ids
        return out


@pytest.mark.gpu
def test_clipwrapper_text_device(cuda, tmp_path, monkeypatch):
    """J: ClipWrapper(text='device') on a tiny checkpoint (visual: width 128, one layer, patch 16, resolution 32; text: width 128, one
    layer): the features within F's bound of text='host'; a wrong-shaped cache file next to the checkpoint is neither read nor
    replaced; on eight random crops the same names and probabilities within 1e-3; encode_prompts gives the class rows."""
    import copy
    from vilgod_amd.clip_wrapper import ClipWrapper
    from vilgod_amd.pipeline import default_preprocessor_cfg
    monkeypatch.setattr(clip_text, 'tokenize_prompts', _WordTokenizer.tokenize_prompts)
    text_sd = cw.synthetic_text_weights(1, width=128, layers=1, embed=64)
    sd = {**{'visual.' + k: v for k, v in cw.synthetic_vit_weights(0, width=128, layers=1, heads=2, patch=16, resolution=32, output_dim=64).items()},
          **text_sd}
    cfg = copy.deepcopy(default_preprocessor_cfg())['clip']
    cfg['model_name'] = 'ViT-tiny.pt'
    host_dir, dev_dir = tmp_path / 'host', tmp_path / 'device'
    for d in (host_dir, dev_dir):
        d.mkdir()
        torch.save(sd, d / 'ViT-tiny.pt')
    stale = dev_dir / 'ViT-tiny.pt.text_features.npy'
    np.save(str(stale), np.ones((3, 5), np.float32))
    before = stale.read_bytes()
    host = ClipWrapper(cfg, str(host_dir), device=cuda, dtype='f32')
    dev = ClipWrapper(cfg, str(dev_dir), device=cuda, dtype='f32', text='device')
    assert (host_dir / 'ViT-tiny.pt.text_features.npy').exists()
    assert stale.read_bytes() == before and sorted(p.name for p in dev_dir.iterdir()) == ['ViT-tiny.pt', 'ViT-tiny.pt.text_features.npy']
    n_cls = len(cfg['class_list'])
    assert dev.text_features.shape == host.text_features.shape == (n_cls, 64)
    # F's bound on the unnormalised features: 8 e_host against float64, on this tower and these prompts
    prompts = [cfg['prompt_template'].format(c) for c in cfg['class_list']]
    tok = _WordTokenizer.tokenize_prompts(prompts)
    f64 = TR.encode_text_f64(text_sd, tok)
    e_host = float((clip_text.encode_text(text_sd, tok).double() - f64).abs().max())
    norm = f64.norm(dim=-1, keepdim=True)
    e_dev = float(((dev.text_features.cpu().double() - f64 / norm) * norm).abs().max())
    print(f"ClipWrapper(text='device'): e_dev {e_dev:.2e}, e_host {e_host:.2e}")
    assert e_dev <= 8 * e_host
    assert float((dev.text_features - host.text_features).abs().max()) <= BAR
    assert torch.equal(dev.encode_prompts(prompts), dev.text_features)
    via = clip_text.text_features(str(dev_dir / 'ViT-tiny.pt'), prompts, device=cuda, tower='device')
    assert np.abs(via - dev.text_features.cpu().numpy()).max() <= 1e-6          # (the same rows, normalised on the host: an ulp or two)
    crops = (torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 1.2).to(cuda)
    names_h, _ = host.predict_clip_labels(crops)
    names_d, _ = dev.predict_clip_labels(crops)
    ph, pd = host.predict_probs(crops)[0], dev.predict_probs(crops)[0]
    assert names_h == names_d and float((ph - pd).abs().max()) <= 1e-3
