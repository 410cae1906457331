"""A unit's result depends on that unit alone: the rows of the projection GEMMs, the items of the attention kernels, the crops of
vg_vit_encode and the feature rows of the scores kernels, each run with every other unit replaced by poison (quiet NaN, +-Inf
alternating, the largest finite value of the buffer's type; tests/independence_ref.py) under two complementary masks, so that every
clean unit has poisoned neighbours on both sides and every 256-row tile that holds two units holds poison.

Every comparison is of bits, between the run with poisoned neighbours and the run of the SAME launch shape whose neighbours are clean
(independence_ref.assert_clean_equal).  So that "consistently wrong" cannot pass, the clean run is also held to the float64 reference
and the bound the existing test of that kernel uses, unchanged: gemm_ref.check_case, gemm_ln_ref's checkers, attention_ref.check under
bound_f16 / bound_f32 (text_tower_ref.causal_reference for the causal kernels), oracle.vit_oracle under test_vit's feature and
probability bars, clip_scores_ref under 1e-5.  No bound of its own.  Each test also asserts that the poisoned units' outputs changed:
poison in bytes nobody reads would prove nothing.

Position and count (vg_vit_encode).  Encoding a permuted batch gives the permuted features, and encode(batch[:m]) equals
encode(batch)[:m] for every m whose plan (stream form and class-row last block, independence_ref.plan) equals n's: no kernel's per-row
arithmetic depends on the row's place in a tile, on the tile's place in the grid or on the workgroup that runs it, and the class-row
compaction keeps row i for crop i.  Both hold on every tower, form and input kind below; nothing had to be narrowed.  Under
VG_GEMM_SPLITK=8 only the companions property is asserted: which rows are tail rows depends on the crop count and on the crop's
position, and a tail row's K-split partial sums are rounded differently from a main row's single accumulation (legitimately: both are
within the GEMM's bound)."""
import ctypes
import functools
import zlib

import pytest
import torch

import attention_ref as A
import clip_scores_ref as CS
import gemm_ln_ref as LN
import gemm_ref as G
import independence_ref as I
import text_tower_ref as TR
import vit_stages_ref as VS
from oracle import vit_oracle as vo
from test_gemm_ln import _check_resid_rows, _consumer_operands, _ln, _producer_operands, sample_rows
from test_vit import SMALL_TOWER
from test_vit_stages import PAIR_TOWER, STREAM_FORMS
from vilgod_amd import clip_weights as cw

VG_OK = 0
GRANS = (1, 32, 197)                       # rows per unit of the GEMM row masks
ENV = {'VG_GEMM_W4': '1', 'VG_GEMM_F32_MFMA': '1'}
NAN = float('nan')


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _set_env(monkeypatch, env):
    for k, v in {**ENV, **dict(env)}.items():
        monkeypatch.setenv(k, v)


def _masks(M):
    """(granularity, phase, clean rows) of a launch of M rows: every granularity that leaves more than one unit, both phases."""
    return [(gran, phase, I.row_mask(M, gran, phase)) for gran in GRANS if gran < M for phase in (0, 1)]


# =================================================================================================================== 1. GEMM rows
def _gemm_cases():
    out = []

    def add(family, shapes, epis, **env):
        for shape in shapes:
            for epi in epis:
                out.append(pytest.param(family, shape, epi, tuple(sorted(env.items())),
                                        id='-'.join([family, 'x'.join(map(str, shape)), f'epi{epi}'] + [f'{k[3:].lower()}{v}' for k, v in sorted(env.items())])))
    # the smallest shape each family takes (test_gemm_families' table)
    add('f16', [(256, 128, 32)], (0, 1, 2, 3))
    add('pp64', [(256, 256, 128)], (0, 1, 2, 3, 4), VG_GEMM_W4='0')
    add('pp64', [(256, 256, 256)], (4,), VG_GEMM_W4='1')
    add('w4', [(256, 256, 256)], (0, 1, 2, 3), VG_GEMM_W4='1')
    add('f32', [(64, 64, 16)], (0, 1, 2, 3))
    add('f32_mfma', [(128, 128, 16)], (0, 1, 2, 3))
    add('f32', [(128, 128, 16)], (0, 1, 2, 3), VG_GEMM_F32_MFMA='0')
    # K no multiple of 256, two row tiles
    add('w4', [(512, 768, 320)], (0, 1, 2, 3), VG_GEMM_W4='1')
    add('pp64', [(512, 768, 320)], (0, 1, 2, 3, 4), VG_GEMM_W4='0')
    # 260 tiles on the persistent grid: a workgroup's second tile starts from pieces prefetched beside poison
    add('w4', [(66560, 256, 256)], (0, 1, 2, 3), VG_GEMM_W4='1')
    return out


GEMM_CASES = _gemm_cases()
LN_CASES = [('w4', kind, shape) for kind in (0, 1) for shape in ((256, 256, 256), (512, 768, 384), (66560, 256, 256))] + \
           [('pp64', kind, shape) for kind in (0, 1) for shape in ((256, 256, 256), (512, 768, 512))] + \
           [('w4', kind, shape) for kind in (2, 3) for shape in ((256, 256, 256), (512, 768, 320), (66560, 256, 256))] + \
           [('pp64', 2, shape) for shape in ((256, 256, 256), (512, 768, 320))]
GEMM_ROWS = sorted({p.values[1][0] for p in GEMM_CASES} | {s[0] for _, _, s in LN_CASES} | {257 * 256})


@functools.lru_cache(maxsize=2)
def _operands(kind, M, N, K, dtype):
    return G.operands(kind, M, N, K, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('family,shape,epi,env', GEMM_CASES)
def test_gemm_rows(cuda, family, shape, epi, env, monkeypatch):
    """vg_gemm: X rows (and the matching resid / resid16 rows of epilogues 2 / 4) poisoned by row masks of 1, 32 and 197 rows; the
    output rows of clean X rows equal the clean run.  Clean run: gemm_ref.check_case (the large launch on test_gemm's integer
    operands and sampled rows: exact)."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    _set_env(monkeypatch, env)
    dtype = G.family_dtype(family)
    M, N, K = shape
    assert lib.vg_gemm_family(dtype, epi, M, N, K) == G.FAMILY_CODES[family]
    large = M > 4096
    o = _operands('integer' if large else 'gauss', M, N, K, dtype)
    d = o.to(cuda)
    c_dtype = torch.float32 if (epi == 3 or dtype == 0) else torch.float16

    def run(X, resid, resid16):
        C = torch.full((M, N), NAN, dtype=c_dtype, device=cuda)
        R = resid16.clone() if epi == 4 else resid.clone() if epi == 2 else torch.full((1,) if large else (M, N), NAN, device=cuda)
        assert lib.vg_gemm(dtype, epi, ptr(X), ptr(d.W), ptr(d.bias), ptr(C), ptr(R), M, N, K, stream_ptr()) == VG_OK
        torch.cuda.synchronize()
        return R if epi in (2, 4) else C

    want = run(d.X, d.resid, d.resid16)
    if large:
        rows = sample_rows(M, G.gen('rows', M))
        assert bool(torch.isfinite(want.float()).all())
        G.check_case(want[rows.to(cuda)].cpu(), o.rows(rows), epi, family)
    else:
        G.check_case(want.cpu(), o, epi, family)
    for gran, phase, clean in _masks(M):
        clean = clean.to(cuda)
        for kind in I.POISONS:
            got = run(I.with_poison(d.X, clean, kind), I.with_poison(d.resid, clean, kind) if epi == 2 else d.resid,
                      I.with_poison(d.resid16, clean, kind) if epi == 4 else d.resid16)
            what = f'{family} {shape} epi {epi} rows of {gran} phase {phase} {kind}'
            I.assert_clean_equal(got, want, clean, what)
            I.assert_poison_arrived(got, want, clean, what)


@pytest.mark.gpu
@pytest.mark.parametrize('family,kind,shape', LN_CASES)
def test_gemm_ln_rows(cuda, family, kind, shape, monkeypatch):
    """vg_gemm_ln.  Kinds 0 / 1 (consumer): X rows and the incoming statistics of the same rows poisoned; C rows of clean rows equal
    the clean run (clean run: gemm_ln_ref.check_consumer_formula).  Kinds 2 / 3 (producers): X rows and the stream's rows (resid, or the
    pair hi / lo) poisoned; the new stream, its fp16 copy and the written statistics of clean rows equal the clean run (clean run:
    check_producer_f32 and the residual bound of test_gemm_ln, resp. check_pair against kind 2 on hi + lo)."""
    monkeypatch.setenv('VG_GEMM_W4', '1' if family == 'w4' else '0')
    from vilgod_amd._lib import lib
    P = lib.vg_gemm_ln_partial_cols()
    assert P == (128 if family == 'w4' else 256)
    M, N, K = shape
    g = G.gen('independence-ln', family, kind, shape)
    rows = sample_rows(M, g).to(cuda) if M > 4096 else torch.arange(M, device=cuda)
    if kind < 2:
        x, gam, beta, W32, b, Wf, c1, c2, parts = _consumer_operands(M, N, K, P, cuda, g)
        X16 = x.half()

        def run(X, st):
            C = torch.full((M, N), NAN, dtype=torch.float16, device=cuda)
            assert _ln(kind, X, Wf, c2, c1, st, C, N, None, None, M, N, K) == VG_OK
            return (C,)
        inputs = (X16, parts)
        want = run(*inputs)
        assert bool(torch.isfinite(want[0]).all())
        LN.check_consumer_formula(want[0][rows], X16[rows], Wf, c1, c2, parts[rows], P, kind == 1)
    else:
        X, W, bias, x, _ = _producer_operands(M, N, K, cuda)

        def run2(Xr, stream):
            resid = stream.clone()
            x16 = torch.full((M, N), NAN, dtype=torch.float16, device=cuda)
            stats = torch.full((M, N // P, 2), NAN, device=cuda)
            assert _ln(2, Xr, W, bias, None, stats, None, N, resid, x16, M, N, K) == VG_OK
            return resid, x16, stats
        if kind == 2:
            run, inputs = run2, (X, x)
            want = run(*inputs)
            LN.check_producer_f32(*want, P)
            _check_resid_rows(want[0], x, X, W, bias, rows)
        else:
            hi, lo = LN.make_pair(x)

            def run(Xr, h, l):
                h2, l2 = h.clone(), l.clone()
                stats = torch.full((M, N // P, 2), NAN, device=cuda)
                assert _ln(3, Xr, W, bias, None, stats, None, N, l2, h2, M, N, K) == VG_OK
                return h2, l2, stats
            inputs = (X, hi, lo)
            want = run(*inputs)
            LN.check_pair(*want, run2(X, hi.float() + lo.float())[0], P)
    for gran, phase, clean in _masks(M):
        clean = clean.to(cuda)
        for pk in I.POISONS:
            got = run(*[I.with_poison(t, clean, pk) for t in inputs])
            for i, (a, b_) in enumerate(zip(got, want)):
                what = f'{family} kind {kind} {shape} output {i} rows of {gran} phase {phase} {pk}'
                I.assert_clean_equal(a, b_, clean, what)
                I.assert_poison_arrived(a, b_, clean, what)


@pytest.mark.gpu
def test_gemm_splitk_tail_rows(cuda, monkeypatch):
    """vg_gemm_resid_splitk, test_gemm_resid_splitk_tail's case of 257 row tiles, K = 3072, VG_GEMM_SPLITK=8: the row tiles behind the
    last complete round run K-split through scratch.  The row masks alternate through the main rows and the tail rows alike.  Clean
    run: that test's bar against the float32 matmul, and its own check that the tail rows were split (they differ from the unsplit
    launch, the main rows do not)."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows_t, K, N = 257, 3072, 768
    M = rows_t * 256
    g = torch.Generator().manual_seed(rows_t + K)
    X = (torch.randn(M, K, generator=g) * 0.5).half().to(cuda)
    W = torch.randn(N, K, generator=g) * 0.05
    W[:, 0] += torch.arange(N) * 1e-3
    W = W.half().to(cuda)
    bias = (torch.randn(N, generator=g) * 0.1).to(cuda)
    resid = torch.randn(M, N, generator=g).to(cuda)
    scratch = torch.empty(64 << 20, dtype=torch.uint8, device=cuda)
    monkeypatch.setenv('VG_GEMM_W4', '0')

    def run(Xr, r, splitk='8'):
        monkeypatch.setenv('VG_GEMM_SPLITK', splitk)
        R = r.clone()
        assert lib.vg_gemm_resid_splitk(ptr(Xr), ptr(W), ptr(bias), ptr(R), M, N, K, ptr(scratch), scratch.numel(), stream_ptr()) == VG_OK
        torch.cuda.synchronize()
        return R
    want = run(X, resid)
    ref = resid + X.float() @ W.float().t() + bias
    assert (want - ref).abs().max().item() < 3e-3 * max(1.0, ref.abs().max().item())
    del ref
    full = rows_t * 3 // n_cu
    r_main = full * n_cu // 3
    tail = (rows_t - r_main) * 3
    assert full >= 1 and 0 < tail <= n_cu // 2, 'this device does not split the case'
    unsplit = run(X, resid, '0')
    assert torch.equal(want[:r_main * 256], unsplit[:r_main * 256]) and not torch.equal(want[r_main * 256:], unsplit[r_main * 256:])
    del unsplit
    for gran, phase, clean in _masks(M):
        clean = clean.to(cuda)
        assert bool(clean[r_main * 256:].any()) and not bool(clean[r_main * 256:].all()) and not bool(clean[:r_main * 256].all())
        for kind in I.POISONS:
            got = run(I.with_poison(X, clean, kind), I.with_poison(resid, clean, kind))
            what = f'split-K rows of {gran} phase {phase} {kind}'
            I.assert_clean_equal(got, want, clean, what)
            I.assert_poison_arrived(got, want, clean, what)


# =================================================================================================================== 2. attention items
ATT_T = (5, 17, 50, 197, 224, 225, 257)                       # 224: the largest T of the short kernel (AT_MAXT)
ATT_KERNELS = {'f16': (1, False, 1024), 'f32': (0, False, 282), 'causal16': (1, True, 224), 'causal32': (0, True, 282)}    # dtype, causal, largest T
ATT_CASES = [(k, T, 5) for k, (_, _, tmax) in ATT_KERNELS.items() for T in ATT_T if T <= tmax] + \
            [(k, 17, 300) for k in ATT_KERNELS]              # 600 items: more than the persistent grid serves in one pass


def _item_columns(n, H, by, phase):
    """bool [n, 64 H]: the output columns of clean items (crop, head), alternating by crop or by head."""
    crop = I.unit_mask(n, phase) if by == 'crop' else torch.ones(n, dtype=torch.bool)
    head = I.unit_mask(H, phase) if by == 'head' else torch.ones(H, dtype=torch.bool)
    return (crop[:, None] & head[None, :]).repeat_interleave(64, dim=1)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel,T,n', ATT_CASES)
def test_attention_items(cuda, kernel, T, n):
    """vg_attention_rows (fp16 with q_tiles 1 and all, fp32) and vg_attention_causal_rows (both types): items (crop, head) alternate between
    clean and poisoned q, k, v, by crop and in a second run by head; the padding columns hold NaN in every run (attention_ref.make_qkv).
    The output columns of clean items equal the clean run; the guard rows around `out` and the rows behind the first query tile of a
    q_tiles = 1 launch keep their prefill.  Clean run: attention_ref.check under bound_f16 / bound_f32."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    dtype, causal, _ = ATT_KERNELS[kernel]
    W, H = 128, 2
    f32 = dtype == 0
    ld = 3 * W if f32 else 3 * W + 64
    fams = [('gauss', 'sink')[c % 2] for c in range(n)]
    qkv, _ = A.make_qkv(fams, n, T, W, H, ld, _seed(kernel, T, n), torch.float32 if f32 else torch.float16)
    ref, Aw = (TR.causal_reference if causal else A.reference)(qkv, n, T, W, H)
    bnd = (A.bound_f32 if f32 else A.bound_f16)(qkv, n, T, W, H, ref, Aw, 1.0)
    d_qkv = qkv.to(cuda)

    def run(d_in, q_tiles):
        buf = A.guarded_out(n * T, W, qkv.dtype, cuda)
        out = ctypes.c_void_p(buf.data_ptr() + W * buf.element_size())
        if causal:
            rc = lib.vg_attention_causal_rows(dtype, ptr(d_in), out, n, T, W, H, ld, stream_ptr())
        else:
            rc = lib.vg_attention_rows(dtype, ptr(d_in), out, n, T, W, H, ld, q_tiles, stream_ptr())
        torch.cuda.synchronize()
        assert rc == VG_OK
        return buf

    for q_tiles in sorted({1 if kernel == 'f16' else A.n_tiles(T), A.n_tiles(T)}):
        want = run(d_qkv, q_tiles)
        A.check(want, ref, bnd, n, T, q_tiles if q_tiles < A.n_tiles(T) else None, f'{kernel} T {T} q_tiles {q_tiles}')
        computed = (torch.arange(T) < 32 * q_tiles).repeat(n)                                    # [n T]: rows the launch owns
        owned = torch.cat([torch.zeros(1, dtype=torch.bool), computed, torch.zeros(1, dtype=torch.bool)]).to(cuda)
        for by in ('crop', 'head'):
            for phase in (0, 1):
                cols = _item_columns(n, H, by, phase)                                            # [n, W]
                clean_in = torch.cat([cols] * 3 + [torch.ones(n, ld - 3 * W, dtype=torch.bool)], 1).repeat_interleave(T, dim=0).to(cuda)
                clean_out = (cols.repeat_interleave(T, dim=0) & computed[:, None]).to(cuda)
                poisoned_out = (~cols.repeat_interleave(T, dim=0) & computed[:, None]).to(cuda)
                for kind in I.POISONS:
                    got = run(I.with_poison(d_qkv, clean_in, kind), q_tiles)
                    what = f'{kernel} T {T} n {n} q_tiles {q_tiles} by {by} phase {phase} {kind}'
                    I.assert_clean_equal(got[1:-1], want[1:-1], clean_out, what)
                    I.assert_poison_arrived(got[1:-1], want[1:-1], ~poisoned_out, what)
                    assert torch.equal(I.bits(got[~owned]), I.bits(want[~owned])), f'{what}: rows no item owns were written'


# =================================================================================================================== 3. crops of vg_vit_encode
def _tower(**kw):
    return dict(kw, layers=2, heads=kw['width'] // 64)


TOWERS = {          # name -> (config, one crop count below and one above the first with the fp16-pair stream)
    'small': (dict(SMALL_TOWER), (60, 105)),                                                       # T = 5
    'pair': (_tower(**PAIR_TOWER), (30, 33)),                                                      # T = 17
    'b16': (dict(cw.VIT_B16, layers=2), (2, 5)),                                                   # T = 197
    'b32': (dict(cw.VIT_B32, layers=2), (10, 13)),                                                 # T = 50
    'l14': (dict(cw.VIT_L14, layers=2), (1, 3)),                                                   # T = 257, K 588 padded to 640
    'w384': (_tower(width=384, patch=16, resolution=32, output_dim=64), (60, 105)),                # never folded
}
FORM_IDS = ['default', 'hl0', 'cls0-hl0', 'w4-0', 'fold0', 'resid16', 'f32', 'pair-boundary']


def _tokens(cfg):
    return (cfg['resolution'] // cfg['patch']) ** 2 + 1


def _geom(cfg):
    return {k: cfg[k] for k in ('width', 'patch', 'resolution', 'output_dim')}


def _counts(name, form):
    cfg, counts = TOWERS[name]
    if FORM_IDS[form] != 'pair-boundary':
        return counts
    return (VS.pair_stream_from(cfg),) if cfg['width'] % 256 == 0 else ()


ENCODE_CASES = [pytest.param(name, form, id=f'{name}-{FORM_IDS[form]}') for name in TOWERS for form in range(len(FORM_IDS)) if _counts(name, form)]
ENCODE_TN = sorted({(_tokens(TOWERS[name][0]), n) for name in TOWERS for form in range(len(FORM_IDS)) for n in _counts(name, form)})


@functools.lru_cache(maxsize=None)
def _tower_weights(name):
    return cw.synthetic_vit_weights(3, **TOWERS[name][0])


def _kinds(cfg, dtype):
    """The input kinds vit_plan accepts: 2 (patch rows, no K padding) and 3 (single-channel rows, patch^2 a multiple of 128) on fp16 towers."""
    pp = cfg['patch'] ** 2
    return [0, 1] + ([2] if dtype == 'f16' and (3 * pp) % 64 == 0 else []) + ([3] if dtype == 'f16' and pp % 128 == 0 else [])


@functools.lru_cache(maxsize=8)
def _inputs(name, n):
    """Seeded inputs of n crops in the four input kinds (host tensors) and the oracle's features of the crops each kind stands for:
    {kind: (input, features)}.  Kind 2: the im2col rows of the fp16 crops; kind 3: levels / 256 (vit_stages_ref.make_levels)."""
    from vilgod_amd.projection import CLIP_MEAN, CLIP_STD
    cfg = TOWERS[name][0]
    wd, res, ps = _tower_weights(name), cfg['resolution'], cfg['patch']
    crops = torch.randn(n, 3, res, res, generator=torch.Generator().manual_seed(_seed(name, n)))
    with torch.no_grad():
        feat = vo.vit_forward(wd, crops, cfg['heads'])
    out = {0: (crops, feat), 1: (crops.half(), feat)}
    P, Pp = n * (_tokens(cfg) - 1), VS.pad256(n * (_tokens(cfg) - 1))
    if 2 in _kinds(cfg, 'f16'):
        rows = torch.zeros(Pp, 3 * ps * ps, dtype=torch.float16)
        rows[:P] = torch.from_numpy(VS.im2col64(crops.half().numpy(), ps, 3 * ps * ps)).half()
        out[2] = (rows, feat)
    if 3 in _kinds(cfg, 'f16'):
        u, rows = VS.make_levels(_geom(cfg), n, _seed('levels', name, n) % 2 ** 31)
        with torch.no_grad():
            feat3 = vo.vit_forward(wd, torch.from_numpy(VS.levels_as_crops(_geom(cfg), n, u, (CLIP_MEAN, CLIP_STD))), cfg['heads'])
        out[3] = (torch.from_numpy(rows), feat3)
    return out


def _take(data, kind, cfg, idx):
    """The input of the crops `idx` (a list, in that order), in the layout of `kind`."""
    if kind < 2:
        return data[idx].contiguous()
    rpc = _tokens(cfg) - 1
    out = torch.zeros(VS.pad256(len(idx) * rpc), data.shape[1], dtype=data.dtype, device=data.device)
    out[:len(idx) * rpc] = data[:data.shape[0] // rpc * rpc].reshape(-1, rpc, data.shape[1])[idx].reshape(-1, data.shape[1])
    return out


def _clean_units(data, kind, cfg, n, phase):
    """The clean / poison mask over dim 0 of an input: crops (kinds 0 / 1), or their patch rows with the buffer's padding rows behind
    the last crop always poisoned (kinds 2 / 3)."""
    return I.unit_mask(n, phase) if kind < 2 else I.crop_rows(n, _tokens(cfg) - 1, phase, total=data.shape[0])


def _encode(enc, data, kind, n):
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    feat = torch.full((n, enc.cfg['output_dim']), NAN, dtype=torch.float32, device=data.device)
    check(lib.vg_vit_encode(enc._h, ptr(data), kind, n, ptr(enc._workspace(n)), ptr(feat), stream_ptr()), 'vg_vit_encode')
    torch.cuda.synchronize()
    return feat


def _check_against_oracle(feat, want, dtype, what):
    """test_vit's bars: fp16 towers, features within 2e-2 relative L2 of the fp32 oracle; fp32 towers, probabilities over 24 prompts
    within 1e-3."""
    feat = feat.cpu()
    assert bool(torch.isfinite(feat).all()), what
    if dtype == 'f16':
        rel = ((feat - want).norm() / want.norm()).item()
        assert rel < 2e-2, (what, rel)
    else:
        text = cw.synthetic_text_features(0, 24, want.shape[1])
        perr = (vo.clip_probabilities(feat, text) - vo.clip_probabilities(want, text)).abs().max().item()
        assert perr < 1e-3, (what, perr)


@pytest.mark.gpu
@pytest.mark.parametrize('name,form', ENCODE_CASES)
def test_encode_crops(cuda, name, form, monkeypatch):
    """Two-layer towers in every stream form of test_vit_stages.STREAM_FORMS, every input kind the plan accepts, one crop count on each
    side of the pair stream's first ('pair-boundary': that count itself).  Companions: poisoned crops (pixels; for kinds 2 / 3 patch
    rows, and the buffer's padding rows in every poisoned run) leave the clean crops' features unchanged and finite, and a clean encode
    on the workspace the poisoned ones left behind equals the first.  Position: a permuted batch gives the permuted features.  Count:
    encode(batch[:m]) == encode(batch)[:m] for every m with n's plan.  Clean run: the fp32 oracle under test_vit's bars."""
    from vilgod_amd._lib import lib
    from vilgod_amd.clip_wrapper import VitEncoder
    switches, dtype = STREAM_FORMS[form]
    dtype = 'f16' if dtype == 'pair' else dtype
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    cfg = TOWERS[name][0]
    T = _tokens(cfg)
    enc = VitEncoder(_tower_weights(name), dtype=dtype, device=cuda)
    for n in _counts(name, form):
        assert (n * T) % 256 != 0 and n * T > 256                 # no whole number of row tiles, at least two of them
        assert lib.vg_vit_workspace_bytes(enc._h, n) == I.workspace_bytes(_geom(cfg), n, dtype, switches), 'the plan restatement and the handle disagree'
        if FORM_IDS[form] == 'pair-boundary':
            assert I.plan(cfg, n, dtype, switches) == ('pair', True) and I.plan(cfg, n - 1, dtype, switches)[0] == 'fold'
        smaller = I.same_plan_counts(cfg, n, dtype, switches)
        for kind in _kinds(cfg, dtype):
            data, oracle = _inputs(name, n)[kind]
            data = data.to(cuda)
            tag = f'{name} {FORM_IDS[form]} n {n} kind {kind}'
            want = _encode(enc, data, kind, n)
            _check_against_oracle(want, oracle, dtype, tag)
            for phase in (0, 1):
                units = I.unit_mask(n, phase)
                clean = _clean_units(data, kind, cfg, n, phase)
                if bool(clean.all()) or not bool(units.any()):
                    continue                                  # (one crop, CHW input: nothing to poison, or nothing clean)
                for pk in I.POISONS:
                    got = _encode(enc, I.with_poison(data, clean.to(cuda), pk), kind, n)
                    I.assert_clean_equal(got, want, units, f'{tag} phase {phase} {pk}')
                    I.assert_poison_arrived(got, want, units, f'{tag} phase {phase} {pk}')
            I.assert_clean_equal(_encode(enc, data, kind, n), want, torch.ones(n, dtype=torch.bool), f'{tag}: clean encode after the poisoned ones')
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).tolist()
            I.assert_clean_equal(_encode(enc, _take(data, kind, cfg, perm), kind, n), want[perm], torch.ones(n, dtype=torch.bool), f'{tag}: permuted batch')
            for m in smaller:
                I.assert_clean_equal(_encode(enc, _take(data, kind, cfg, list(range(m))), kind, m), want[:m], torch.ones(m, dtype=torch.bool),
                                     f'{tag}: the first {m} crops alone')


@pytest.mark.gpu
def test_encode_crops_with_split_k_tails(cuda, monkeypatch):
    """VG_GEMM_SPLITK=8 on the k_gemm_f16_pp64 family, ViT-B/16 geometry, 334 crops = 258 row tiles (test_vit's split-K case): the
    companions property alone -- tail rows legitimately differ in fp32 rounding from main rows, so neither position nor count is a
    property of this configuration.  Clean run: the fp32 oracle on the first and the last three crops (main rows and tail rows)."""
    from vilgod_amd.clip_wrapper import VitEncoder
    monkeypatch.setenv('VG_GEMM_W4', '0')
    monkeypatch.setenv('VG_GEMM_SPLITK', '8')
    cfg, n = TOWERS['b16'][0], 334
    wd = _tower_weights('b16')
    enc = VitEncoder(wd, dtype='f16', device=cuda)
    crops = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(n)).half()
    some = [0, 1, 2, n - 3, n - 2, n - 1]
    with torch.no_grad():
        oracle = vo.vit_forward(wd, crops[some].float(), cfg['heads'])
    data = crops.to(cuda)
    want = _encode(enc, data, 1, n)
    assert bool(torch.isfinite(want).all())
    _check_against_oracle(want[some], oracle, 'f16', 'split-K tower')
    # the tails really are split here: against a handle made under VG_GEMM_SPLITK=0 the crops with a tail row differ, the others do not
    monkeypatch.setenv('VG_GEMM_SPLITK', '0')
    unsplit = _encode(VitEncoder(wd, dtype='f16', device=cuda), data, 1, n)
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    row_tiles = (n * 197 + 255) // 256
    first_tail_crop = (row_tiles * 3 // n_cu) * n_cu // 3 * 256 // 197
    changed = (I.bits(unsplit) != I.bits(want)).any(dim=1)
    assert bool(changed.any()) and not bool(changed[:first_tail_crop].any()), (int(changed.sum()), first_tail_crop)
    for phase in (0, 1):
        units = I.unit_mask(n, phase)
        for pk in I.POISONS:
            got = _encode(enc, I.with_poison(data, units.to(cuda), pk), 1, n)
            I.assert_clean_equal(got, want, units, f'split-K tower phase {phase} {pk}')
            I.assert_poison_arrived(got, want, units, f'split-K tower phase {phase} {pk}')


# =================================================================================================================== 4. scores rows
@pytest.mark.gpu
@pytest.mark.parametrize('dim', [512, 101])
@pytest.mark.parametrize('n_classes', [1, 24, 64, 65, 257])
def test_scores_rows(cuda, dim, n_classes):
    """vg_clip_scores (up to 64 classes) and vg_clip_scores_wide (above): feature rows of NaN, +-Inf and zeros (norm 0) between the clean
    ones; probs, top1 and score of clean rows equal the clean run.  Clean run: clip_scores_ref.reference, |dp| <= 1e-5 and check_top1."""
    from vilgod_amd.clip_wrapper import clip_scores
    for n in (1, 63, 64, 65, 257):
        g = torch.Generator().manual_seed(CS.seed('independence', dim, n_classes, n))
        feat = torch.randn(n, dim, generator=g)
        text = CS.unit_rows(n_classes, dim, g)
        d_feat, d_text = feat.to(cuda), text.to(cuda)
        want = clip_scores(d_feat, d_text)
        ref = CS.reference(feat, text)
        assert (want[0].cpu().double() - ref).abs().max() <= 1e-5
        if n_classes > 1:
            CS.check_top1(want[0].cpu(), want[1].cpu(), want[2].cpu(), ref)
        for phase in (0, 1):
            clean = I.unit_mask(n, phase)
            if not bool(clean.any()):
                continue
            for kind in I.SCORE_POISONS:
                got = clip_scores(I.with_poison(d_feat, clean.to(cuda), kind), d_text)
                for a, b, what in zip(got, want, ('probs', 'top1', 'score')):
                    I.assert_clean_equal(a, b, clean, f'D {dim} K {n_classes} n {n} phase {phase} {kind} {what}')
                if n_classes > 1:
                    I.assert_poison_arrived(got[0], want[0], clean, f'D {dim} K {n_classes} n {n} phase {phase} {kind}')


# =================================================================================================================== CPU
def test_masks_leave_no_clean_unit_without_poisoned_neighbours():
    """For every row count and granularity of the GEMM tests and every (T, n) of the encode tests, both phases: no clean unit has a clean
    neighbour, no unit is partly poisoned, and every 256-row tile that holds rows of two units holds clean and poisoned rows; the two
    phases are complementary.  (A tile inside ONE unit -- T = 257, rows 0 .. 255 -- is poisoned under the other phase.)"""
    for M in GEMM_ROWS:
        assert _masks(M)
        for gran, phase, clean in _masks(M):
            assert I.mask_gaps(clean, gran) == [], (M, gran, phase)
            assert torch.equal(clean, ~I.row_mask(M, gran, 1 - phase))
    assert (197, 2) in ENCODE_TN and (197, 5) in ENCODE_TN and (257, 1) in ENCODE_TN and (257, 3) in ENCODE_TN and (50, 10) in ENCODE_TN and (50, 13) in ENCODE_TN
    for T, n in ENCODE_TN:
        assert (n * T) % 256 != 0, (T, n)
        for phase in (0, 1):
            assert I.mask_gaps(I.crop_rows(n, T, phase), T) == [], (T, n, phase)
            rows = I.crop_rows(n, T - 1, phase, total=VS.pad256(n * (T - 1)))
            assert I.mask_gaps(rows, T - 1) == [] and not bool(rows[n * (T - 1):].any()), (T, n, phase)
    # the check has teeth
    two_clean = torch.tensor([True] * 8 + [False] * 4)
    assert I.mask_gaps(two_clean, 4) == ['clean units 0 and 1 are neighbours']
    assert I.mask_gaps(torch.tensor([True, True, False, True]), 2) == ['unit 1 is partly poisoned']
    assert any('tile at row 256' in s for s in I.mask_gaps(torch.ones(600, dtype=torch.bool), 300))
    assert 257 * 3 > 512 and I.crop_rows(3, 257, 0)[256]          # T = 257, 3 crops: row 256 is crop 0's last row


def test_poison_patterns():
    for dtype in (torch.float16, torch.float32):
        assert bool(torch.isnan(I.poison_row(6, dtype, 'nan')).all())
        inf = I.poison_row(6, dtype, 'inf')
        assert bool(torch.isinf(inf).all()) and bool((inf[0::2] > 0).all()) and bool((inf[1::2] < 0).all())
        assert bool((I.poison_row(6, dtype, 'max') == torch.finfo(dtype).max).all())
    t = torch.arange(12.0).reshape(4, 3)
    p = I.with_poison(t, torch.tensor([True, False, True, False]), 'nan')
    assert torch.equal(p[[0, 2]], t[[0, 2]]) and bool(torch.isnan(p[[1, 3]]).all()) and not bool(torch.isnan(t).any())
    I.assert_clean_equal(p, t, torch.tensor([True, False, True, False]))
    I.assert_poison_arrived(p, t, torch.tensor([True, False, True, False]))
    with pytest.raises(AssertionError):
        I.assert_clean_equal(p, t, torch.tensor([True, True, True, False]))
    with pytest.raises(AssertionError):
        I.assert_poison_arrived(t, t, torch.tensor([True, False, True, False]))
    z = torch.zeros(2, 2)
    with pytest.raises(AssertionError):
        I.assert_clean_equal(-z, z, torch.tensor([True, True]))     # bits, not values


def test_plan_restatement_agrees_with_the_handle_and_with_pair_stream_from():
    """independence_ref.plan: the first crop count with the pair stream is vit_stages_ref.pair_stream_from's on every folded tower, the
    class-row last block starts there too, no switch combination of STREAM_FORMS gives a pair without both; its workspace size is the
    handle's (vg_vit_workspace_bytes: host arithmetic, no device)."""
    from vilgod_amd._lib import lib
    for name, (cfg, counts) in TOWERS.items():
        first = next((n for n in range(1, 400) if I.plan(cfg, n)[0] == 'pair'), None)
        if cfg['width'] % 256:
            assert first is None and {I.plan(cfg, n) for n in range(1, 400)} == {('f32', False)}
            continue
        assert first == VS.pair_stream_from(cfg) and counts[0] < first <= counts[1], (name, first)
        assert I.plan(cfg, first - 1) == ('fold', False) and I.plan(cfg, first) == ('pair', True)
        for switches, dtype in STREAM_FORMS:
            for n in (first - 1, first, first + 7):
                stream, cls = I.plan(cfg, n, 'f16' if dtype == 'pair' else dtype, switches)
                assert (stream == 'pair') == (not switches and dtype != 'f32' and n >= first)
                assert cls == (n >= first and dtype != 'f32' and not ({'VG_VIT_CLS_LAST', 'VG_VIT_LN_FOLD', 'VG_VIT_RESID16'} & set(switches)))
        assert I.same_plan_counts(cfg, first + 2) == [first, first + 1]
    assert VS.pair_stream_from(cw.VIT_B16) == 3 and I.plan(cw.VIT_B16, 2) == ('fold', False) and I.plan(dict(cw.VIT_B16, layers=1), 8) == ('fold', False)
    for name in ('small', 'l14', 'w384'):
        cfg = TOWERS[name][0]
        for dtype in (0, 1):
            h = ctypes.c_void_p()
            assert lib.vg_vit_create(ctypes.byref(h), cfg['width'], cfg['layers'], cfg['heads'], cfg['patch'], cfg['resolution'], cfg['output_dim'], dtype) == VG_OK
            try:
                for n in (1, 3, 60, 105):
                    assert lib.vg_vit_workspace_bytes(h, n) == I.workspace_bytes(_geom(cfg), n, ('f32', 'f16')[dtype])
            finally:
                lib.vg_vit_destroy(h)
