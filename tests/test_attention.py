"""The attention kernels at kernel level (vg_attention_rows; csrc/vit.hip k_attention_f16, k_attention_f16_long, k_attention_f32) against
the float64 softmax(q k^T / 8) v of tests/attention_ref.py, under bounds derived from the kernels' arithmetic (attention_ref.bound_f16 /
bound_f32), on input families that stress what a softmax kernel can get wrong: the maximum ('hot', 'sink', 'sink_last'), the
denominator and the key mask ('uniform'), the key <-> register mapping ('onehot'); at the token counts where the kernels change
instantiation, skip key steps or wrap their persistent loops; with the caller's q_tiles; and with NaN in every byte the kernels must
not read (padding columns) or leave unwritten (out).  The CPU test at the end runs the checker against emulated right and wrong
kernels.  Every case prints its worst |got - want| / bound (pytest -s).  k_clip_scores' shapes and edges are at the bottom."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import attention_ref as R

VG_OK, VG_ERR_ARG = 0, 1
S = 1.0                                # safety factor of the bounds (attention_ref.bound_f16 / bound_f32): 1, at most 2
ATT_VARIANTS = (('1', '1'), ('1', '0'), ('0', '0'))      # (VG_ATT_TR, VG_ATT_STAGGER): the three T = 197 instantiations


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=3)
def _case(family, n_crops, T, W, H, pad, f32=False):
    """Inputs, float64 reference and bound of one case, built once (the variants and q_tiles of a case share it).
    family: a name, or a tuple of names alternating by crop."""
    fams = family if isinstance(family, str) else [family[c % len(family)] for c in range(n_crops)]
    ld = 3 * W + pad
    qkv, perm = R.make_qkv(fams, n_crops, T, W, H, ld, _seed(family, n_crops, T, W, f32), torch.float32 if f32 else torch.float16)
    want, A = R.reference(qkv, n_crops, T, W, H)
    bnd = (R.bound_f32 if f32 else R.bound_f16)(qkv, n_crops, T, W, H, want, A, S)
    return qkv, perm, want, A, bnd, ld


def _rows(dtype, d_qkv, buf, n_crops, T, W, H, ld, q_tiles):
    """vg_attention_rows into the rows between the guard rows of `buf`."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    out = None if buf is None else ctypes.c_void_p(buf.data_ptr() + W * buf.element_size())
    rc = lib.vg_attention_rows(dtype, ptr(d_qkv), out, n_crops, T, W, H, ld, q_tiles, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _run(cuda, family, n_crops, T, W, H, pad=64, f32=False, q_tiles=None, d_qkv=None, what=''):
    """One launch of a case through the checker -> (guarded out buffer on the CPU, worst ratio)."""
    qkv, perm, want, A, bnd, ld = _case(family, n_crops, T, W, H, pad, f32)
    if d_qkv is None:
        d_qkv = qkv.to(cuda)
    buf = R.guarded_out(n_crops * T, W, qkv.dtype, cuda)
    assert _rows(0 if f32 else 1, d_qkv, buf, n_crops, T, W, H, ld, R.n_tiles(T) if q_tiles is None else q_tiles) == VG_OK
    buf = buf.cpu()
    what = f'{what or ("f32" if f32 else "f16")} {family} {n_crops}x{T} W={W}' + (f' q_tiles={q_tiles}' if q_tiles else '')
    worst = R.check(buf, want, bnd, n_crops, T, q_tiles, what)
    if perm is not None and q_tiles is None:
        fams = [family] * n_crops if isinstance(family, str) else [family[c % len(family)] for c in range(n_crops)]
        R.check_onehot(buf, qkv, perm, n_crops, T, W, H, [c for c, f in enumerate(fams) if f == 'onehot'])
    print(f'{what}: worst |got - want| / bound = {worst:.3f}')
    return buf, worst


# ------------------------------------------------------------------------------------------------------------------- fp16, token counts
SHORT = [(T, 768, 12) for T in (1, 2, 31, 32, 33, 64, 96, 128, 160, 192, 193, 197, 224)] + [(50, 256, 4), (197, 256, 4), (50, 512, 8), (197, 512, 8)]
LONG = [(T, 1024, 16) for T in (225, 256, 257, 289, 305, 321, 577, 1000, 1024)] + [(257, 768, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('T,W,H', SHORT)
def test_short_kernel_token_counts(cuda, T, W, H, family):
    """k_attention_f16: every NKB instantiation at its first and last token count (tail 1 and tail 32), the T = 197 one, T = 1 and 2,
    heads 4 / 8 / 12; 3 crops."""
    _run(cuda, family, 3, T, W, H, what='short')


@pytest.mark.gpu
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('T,W,H', LONG)
def test_long_kernel_token_counts(cuda, T, W, H, family):
    """k_attention_f16_long: the first T it takes, no masked key (256, 1024), one key in the last block (257, 321, 577), the 16-key skip
    boundaries (289, 305), an odd number of key blocks with a partial last pass (321: 5 blocks, 11 tiles), T = 1000 (24 masked keys);
    2 crops."""
    _run(cuda, family, 2, T, W, H, what='long')


# ------------------------------------------------------------------------------------------------------------------- persistent loops
@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gauss', 'hot'])
@pytest.mark.parametrize('T', [197, 50])
def test_short_kernel_persistent_loop(cuda, T, family, monkeypatch):
    """54 crops x 12 heads = 648 items on 256 workgroups (2.53 per workgroup, 136 left over): the register prefetch of item
    i + gridDim.x, the LDS reuse behind the end-of-item barrier and has_next, against the reference, under the three instantiations
    the VG_ATT_TR / VG_ATT_STAGGER switches choose at T = 197 (bit-identical with each other).  The crops alternate between `family`
    and 'sink': a stale K / V block would come from different data."""
    n_crops, W, H = 54, 768, 12
    d_qkv = _case((family, 'sink'), n_crops, T, W, H, 64)[0].to(cuda)
    outs = []
    for tr, stag in ATT_VARIANTS:
        monkeypatch.setenv('VG_ATT_TR', tr)
        monkeypatch.setenv('VG_ATT_STAGGER', stag)
        outs.append(_run(cuda, (family, 'sink'), n_crops, T, W, H, d_qkv=d_qkv, what=f'short persistent TR={tr} STAGGER={stag}')[0])
    assert all(torch.equal(outs[0][1:-1].view(torch.int16), o[1:-1].view(torch.int16)) for o in outs[1:])


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['gauss', 'hot'])
def test_long_kernel_persistent_loop(cuda, family):
    """71 crops x 16 heads = 1136 items on at most 512 workgroups (2.2 per workgroup, 112 left over): decode() with u > 0, the prefetch
    across pass and item seams, against the reference; crops alternate between `family` and 'sink'."""
    _run(cuda, (family, 'sink'), 71, 257, 1024, 16, what='long persistent')


# ------------------------------------------------------------------------------------------------------------------- q_tiles
@pytest.mark.gpu
@pytest.mark.parametrize('T,W,H,n_crops', [(197, 768, 12, 22), (257, 1024, 16, 33), (577, 1024, 16, 33)])
def test_q_tiles(cuda, T, W, H, n_crops):
    """The class-row-only launch of the tower's last block (q_tiles = 1) and q_tiles = 2, with more items than persistent workgroups
    (264 on 256, 528 on 512): the written rows are bit-identical to the same rows of the all-rows launch and within the bound of the
    reference, every other row of out keeps its NaN."""
    family = ('gauss', 'sink_last')
    d_qkv = _case(family, n_crops, T, W, H, 64)[0].to(cuda)
    full = _run(cuda, family, n_crops, T, W, H, d_qkv=d_qkv)[0][1:-1].view(torch.int16).reshape(n_crops, T, W)
    for qt in (1, 2):
        part = _run(cuda, family, n_crops, T, W, H, q_tiles=qt, d_qkv=d_qkv)[0][1:-1].view(torch.int16).reshape(n_crops, T, W)
        assert torch.equal(part[:, :32 * qt], full[:, :32 * qt])


# ------------------------------------------------------------------------------------------------------------------- fp32
@functools.lru_cache(maxsize=None)
def _f32_max_tokens():
    """The largest T vg_attention_rows(dtype 0) takes, found from its refusals (one-crop launches on zeros)."""
    dev = torch.device('cuda:0')
    W, H = 768, 12
    qkv = torch.zeros(1024, 3 * W, device=dev)
    T = 257
    while T < 1024:
        buf = R.guarded_out(T + 1, W, torch.float32, dev)
        if _rows(0, qkv, buf, 1, T + 1, W, H, 3 * W, R.n_tiles(T + 1)) != VG_OK:
            assert bool(torch.isnan(buf[1:-1]).all())
            break
        T += 1
    return T


@pytest.mark.gpu
def test_f32_size_limit(cuda):
    """k_attention_f32 keeps K [T][65], V [T][64] and 16 rows of probabilities in its 160 KiB of LDS: T * 145 floats."""
    T = _f32_max_tokens()
    assert T * 145 * 4 <= 160 * 1024 < (T + 1) * 145 * 4, T


@pytest.mark.gpu
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('W,H', [(768, 12), (1024, 16)])
@pytest.mark.parametrize('T', [1, 50, 197, 257, 'max'])
def test_f32_kernel(cuda, T, W, H, family):
    """k_attention_f32 (ld = 3 W: no padding columns) under the fp32 bound; on 'gauss' that bound is at least 10 times tighter than the
    fp16 kernels', element by element -- a kernel that rounded anything to fp16 would not pass."""
    T = _f32_max_tokens() if T == 'max' else T
    _run(cuda, family, 3, T, W, H, pad=0, f32=True)
    if family == 'gauss':
        qkv, _, want, A, bnd, _ = _case(family, 3, T, W, H, 0, True)
        tighter = (R.bound_f16(qkv, 3, T, W, H, want, A) / bnd).min().item()
        print(f'f32 gauss T={T}: the fp16 bound is >= {tighter:.1f} x the fp32 bound')
        assert tighter >= 10.0


@pytest.mark.gpu
def test_f32_kernel_many_items(cuda):
    """40 crops x 12 heads: one workgroup per item."""
    _run(cuda, ('gauss', 'sink'), 40, 197, 768, 12, pad=0, f32=True)


# ------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_rejections(cuda):
    """Arguments no kernel serves: VG_ERR_ARG and nothing launched (out keeps its NaN)."""
    W, H = 768, 12
    for dtype, td, pad in ((1, torch.float16, 64), (0, torch.float32, 0)):
        ld = 3 * W + pad
        qkv = torch.zeros(2 * 1025, ld, dtype=td, device=cuda)
        buf = R.guarded_out(2 * 1025, W, td, cuda)
        bad = [dict(T=0), dict(T=1025, q_tiles=33), dict(T=1025, q_tiles=32), dict(H=11), dict(H=13), dict(q_tiles=0), dict(q_tiles=8),
               dict(q_tiles=-1), dict(qkv=None), dict(buf=None), dict(n_crops=0), dict(dtype=2), dict(ld=3 * W - 8)]
        if dtype == 0:
            bad += [dict(ld=3 * W + 64), dict(q_tiles=1), dict(T=_f32_max_tokens() + 1, q_tiles=R.n_tiles(_f32_max_tokens() + 1)),
                    dict(T=577, q_tiles=19)]
        for kw in bad:
            a = dict(dtype=dtype, qkv=qkv, buf=buf, n_crops=2, T=197, W=W, H=H, ld=ld, q_tiles=7)
            a.update(kw)
            assert _rows(a['dtype'], a['qkv'], a['buf'], a['n_crops'], a['T'], a['W'], a['H'], a['ld'], a['q_tiles']) == VG_ERR_ARG, kw
        assert bool(torch.isnan(buf[1:-1]).all()) and bool((buf[0] == R.GUARD).all())


# ------------------------------------------------------------------------------------------------------------------- the checker (CPU)
EMUL_T = (1, 2, 31, 32, 33, 64, 197, 224, 225, 257, 577, 1024)


def _rejected(out, want, bnd, n, T):
    try:
        R.check(R.as_guarded(out), want, bnd, n, T)
    except AssertionError:
        return True
    return False


def test_checker_accepts_the_emulated_kernels_and_rejects_synthesised_faults():
    """Without a GPU: the CPU emulation of the kernels' rounding (one pass, and 64-key online blocks) passes the checker on every
    family at every T; the output of each of these wrong kernels is rejected on at least one family at every T where the fault can
    be expressed:
      (a) 'halfmax'  the cross-half maximum shuffle left out             (T >= 5: below, one lane half holds every key)
      (b) 'padsum'   the key >= T mask of the last block left out        (T not a multiple of the key block)
      (c) 'stale'    one 32-key block of K and V from the previous item  (every T)
      (d) 'vswap'    two keys of V exchanged, K in place                 (T >= 2)
      (e) 'noalpha'  the online rescale left out at one block            (online blocks, T > 64)
      (f) want + 1.9e-3 max|v| on one element per row, on 'gauss': an error the flat bound 2e-3 max|v| of the older tests let pass
    and rows, guard rows or NaN where they must not be are rejected too.  The worst accepted ratio is printed: 0.47 over these cases."""
    W, H, n = 128, 2, 2
    worst = 0.0
    for T in EMUL_T:
        caught = {}
        for fam in R.FAMILIES:
            qkv, _ = R.make_qkv(fam, n, T, W, H, 3 * W + 8, _seed('emul', fam, T))
            want, A = R.reference(qkv, n, T, W, H)
            bnd = R.bound_f16(qkv, n, T, W, H, want, A, S)
            for blk in (None, 64):
                worst = max(worst, R.check(R.as_guarded(R.emulate(qkv, n, T, W, H, blk)), want, bnd, n, T, what=f'emulation {fam} T={T} blk={blk}'))
                if T > 224 if blk is None else T <= 64:          # faults in the mode of the kernel that serves this T (online: also 64 < T <= 224)
                    continue
                faults = [('stale', 0)] + [('stale', (T - 1) // 32)] * (T > 32)
                if T >= 5:
                    faults.append(('halfmax', 0))
                if T % (blk or 32):
                    faults.append(('padsum', 0))
                if T >= 2:
                    faults += [('vswap', 0)] + [('vswap', (T - 2) // 32)] * (T > 33)
                if blk and T > 64:
                    faults += [('noalpha', 0), ('noalpha', (T - 1) // 64 - 1)]
                for f, b in faults:
                    if _rejected(R.emulate(qkv, n, T, W, H, blk, f, b), want, bnd, n, T):
                        caught.setdefault((f, b, blk), []).append(fam)
                    else:
                        caught.setdefault((f, b, blk), [])
            if fam == 'gauss':
                off = want.clone()
                vmax = qkv[:, 2 * W:3 * W].double().abs().max().item()
                off[:, 5] += 1.9e-3 * vmax
                assert (off - want).abs().max() < R.FLAT_OLD * vmax                                   # (f): the flat bound accepts it
                assert _rejected(off.half(), want, bnd, n, T), f'(f) accepted at T={T}'
        missed = [k for k, fams in caught.items() if not fams]
        assert not missed, f'T={T}: faults no family rejects: {missed}'
    print(f'worst accepted emulation ratio {worst:.3f}')
    assert worst <= 0.6                                                                          # (the bound is not loose by design)
    # the structural checks
    T, qt = 70, 1
    qkv, _ = R.make_qkv('gauss', n, T, W, H, 3 * W, 1)
    want, A = R.reference(qkv, n, T, W, H)
    bnd = R.bound_f16(qkv, n, T, W, H, want, A, S)
    out = R.emulate(qkv, n, T, W, H)
    R.check(R.as_guarded(out, qt, T), want, bnd, n, T, qt)
    with pytest.raises(AssertionError, match='beyond query tile'):
        R.check(R.as_guarded(out), want, bnd, n, T, qt)                      # rows beyond the tile written
    with pytest.raises(AssertionError, match='not finite'):
        R.check(R.as_guarded(out, qt, T), want, bnd, n, T)                   # rows left unwritten
    for row in (0, -1):
        buf = R.as_guarded(out)
        buf[row, 3] = 0.0
        with pytest.raises(AssertionError, match='guard'):
            R.check(buf, want, bnd, n, T)
    # 'onehot' exactness: a neighbouring key's value row is not accepted
    qkv, perm = R.make_qkv('onehot', n, 40, W, H, 3 * W, 2)
    out = R.emulate(qkv, n, 40, W, H)
    R.check_onehot(R.as_guarded(out), qkv, perm, n, 40, W, H)
    with pytest.raises(AssertionError):
        R.check_onehot(R.as_guarded(R.emulate(qkv, n, 40, W, H, None, 'vswap', 1)), qkv, perm, n, 40, W, H)


def test_f32_bound_is_an_fp32_bound():
    """bound_f32 on 'gauss' is at least 10 times tighter than bound_f16 element by element (else the fp32 test would not test fp32), and
    a float32 torch attention of the same inputs passes it."""
    n, W, H = 2, 128, 2
    for T in (1, 50, 197, 282):
        qkv, _ = R.make_qkv('gauss', n, T, W, H, 3 * W, _seed('f32', T), torch.float32)
        want, A = R.reference(qkv, n, T, W, H)
        b32 = R.bound_f32(qkv, n, T, W, H, want, A, S)
        assert (R.bound_f16(qkv, n, T, W, H, want, A) / b32).min() >= 10.0
        q, k, v = [qkv[:, i * W:(i + 1) * W].reshape(n, T, H, 64).transpose(1, 2) for i in range(3)]
        got = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(n * T, W)
        R.check(R.as_guarded(got), want, b32, n, T)
        assert _rejected(got.half().float(), want, b32, n, T)


# ------------------------------------------------------------------------------------------------------------------- k_clip_scores
def _clip_ref(feat, text):
    f = feat.double()
    return torch.softmax(100.0 * (f / f.norm(dim=-1, keepdim=True)) @ text.double().t(), dim=-1)


def _unit_rows(n, dim, g):
    t = torch.randn(n, dim, generator=g)
    return t / t.norm(dim=-1, keepdim=True)


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [512, 768])
@pytest.mark.parametrize('n_classes', [1, 2, 24, 63, 64])
@pytest.mark.parametrize('scale', [1.0, 1e-4, 1e4])
def test_clip_scores_shapes(cuda, dim, n_classes, scale):
    """k_clip_scores against float64 softmax(100 normalise(feat) text^T): ViT-B and ViT-L/14 feature widths, 1 to 64 classes, features
    far from unit norm; |dp| <= 1e-5, top-1 equal wherever the reference's margin exceeds that."""
    from vilgod_amd.clip_wrapper import clip_scores
    g = torch.Generator().manual_seed(_seed(dim, n_classes))
    feat = torch.randn(37, dim, generator=g) * scale
    text = _unit_rows(n_classes, dim, g)
    want = _clip_ref(feat, text)
    probs, top1, score = (t.cpu() for t in clip_scores(feat.to(cuda), text.to(cuda)))
    assert (probs.double() - want).abs().max() <= 1e-5
    _check_top1(probs, top1, score, want)


def _check_top1(probs, top1, score, want):
    assert torch.equal(score, probs.gather(1, top1.long()[:, None])[:, 0])
    assert bool((probs <= score[:, None]).all())
    if want.shape[1] > 1:
        best2 = want.topk(2, dim=-1).values
        sure = best2[:, 0] - best2[:, 1] > 2e-5
        assert torch.equal(top1.long()[sure], want.argmax(-1)[sure])
    else:
        assert bool((top1 == 0).all()) and bool((probs == 1).all())


@pytest.mark.gpu
def test_clip_scores_refuses_65_classes(cuda):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    feat = torch.randn(4, 512, device=cuda)
    probs = torch.full((4, 65), float('nan'), device=cuda)
    top1 = torch.full((4,), -7, dtype=torch.int32, device=cuda)
    score = torch.full((4,), float('nan'), device=cuda)
    for K in (65, 0):
        text = _unit_rows(max(K, 1), 512, torch.Generator().manual_seed(0)).to(cuda)
        assert lib.vg_clip_scores(ptr(feat), 4, 512, ptr(text), K, ptr(probs), ptr(top1), ptr(score), stream_ptr()) == VG_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(probs).all()) and bool((top1 == -7).all())


@pytest.mark.gpu
def test_clip_scores_exact_tie(cuda):
    """Two identical text rows: the same probability, bit for bit, and the lower index wins where they are the best."""
    from vilgod_amd.clip_wrapper import clip_scores
    g = torch.Generator().manual_seed(3)
    text = _unit_rows(24, 512, g)
    text[17] = text[5]
    feat = torch.randn(64, 512, generator=g)
    feat[:32] += 3.0 * text[5] * feat[:32].norm(dim=-1, keepdim=True)          # rows whose best class is the tied pair
    want = _clip_ref(feat, text)
    probs, top1, score = (t.cpu() for t in clip_scores(feat.to(cuda), text.to(cuda)))
    assert (probs.double() - want).abs().max() <= 1e-5
    assert torch.equal(probs[:, 5], probs[:, 17])
    assert bool((top1[:32] == 5).all()) and bool((top1 != 17).all())
    assert torch.equal(score[:32], probs[:32, 5])


@pytest.mark.gpu
def test_clip_scores_5000_crops(cuda):
    from vilgod_amd.clip_wrapper import clip_scores
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(5000, 768, generator=g)
    text = _unit_rows(24, 768, g)
    want = _clip_ref(feat, text)
    probs, top1, score = (t.cpu() for t in clip_scores(feat.to(cuda), text.to(cuda)))
    assert (probs.double() - want).abs().max() <= 1e-5
    _check_top1(probs, top1, score, want)
