"""The folded-LayerNorm epilogues of the fp16 projection GEMM at kernel level (vg_gemm_ln; csrc/vit.hip k_gemm_f16_w4 and k_gemm_f16_pp64,
LN = 1 / 2, EPI_BIAS_RESID_HL) against the plain float64 references of tests/gemm_ln_ref.py, both kernel families where they exist.

Exact where the arithmetic is exact: the producer's fp32 stream equals vg_gemm's residual epilogue bit for bit, its fp16 copy is f16 of it,
the pair producer's hi / lo equal f16 of the fp32 stream and of its remainder.  Bounded where fp32 rounding enters: the partial statistics
(2e-6 mean|v| / 1e-5 relative), the consumer (one fp16 ulp + an fp32 error bound per element, gemm_ln_ref.consumer_formula).  The largest
deviations are printed (pytest -s)."""
import zlib

import pytest
import torch

import gemm_ln_ref as R

FAMILIES = {'w4': '1', 'pp64': '0'}
VG_OK, VG_ERR_ARG = 0, 1


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _weights(N, K, gen):
    W = torch.randn(N, K, generator=gen) * 0.05
    W[:, 0] += torch.arange(N) * 1e-3                  # asymmetric, non-identity (a transposed tile must not pass)
    return W


def _ln(kind, X, W, bias, c1, stats, C, ldc, resid, x16, M, N, K, c_off=0):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    import ctypes
    cp = None if C is None else ctypes.c_void_p(C.data_ptr() + c_off * C.element_size())
    rc = lib.vg_gemm_ln(kind, ptr(X), ptr(W), ptr(bias), ptr(c1), ptr(stats), cp, ldc, ptr(resid), ptr(x16), M, N, K, stream_ptr())
    torch.cuda.synchronize()
    return rc


def _cols():
    from vilgod_amd._lib import lib
    return lib.vg_gemm_ln_partial_cols()


def sample_rows(M, gen, per_tile=(0, 63, 64, 127, 128, 191, 192, 255), n_random=256):
    """Rows of a large launch to check against float64: in EVERY 256-row tile the first and last row of each 64-lane group (both
    halves wm of a w4 workgroup, both lane halves h of its statistics prefetch) -- so the first and last tile of every persistent
    workgroup are among them -- plus random rows."""
    base = torch.arange(0, M, 256)[:, None] + torch.tensor(per_tile)[None, :]
    return torch.unique(torch.cat([base.flatten(), torch.randint(0, M, (n_random,), generator=gen)]))


def _set_family(monkeypatch, family):
    monkeypatch.setenv('VG_GEMM_W4', FAMILIES[family])
    assert _cols() == (128 if family == 'w4' else 256)


# ------------------------------------------------------------------------------------------------------------------- producers
PRODUCER_SHAPES = [(256, 256, 256), (768, 256, 1024), (512, 512, 512), (512, 768, 768), (256, 768, 3072), (512, 1024, 1024),
                   (256, 1024, 4096), (64256, 768, 768), (65792, 768, 768)]      # (M, W, K): one tile, three tiles, out_proj / c_proj per width, 251 / 257 row tiles


def _producer_operands(M, N, K, cuda):
    g = _gen('producer', M, N, K)
    X = (torch.randn(M, K, generator=g) * 0.5).half().to(cuda)
    W = _weights(N, K, g).half().to(cuda)
    bias = (torch.randn(N, generator=g) * 0.1).to(cuda)
    x = R.ln_rows(M, N, g).to(cuda)
    return X, W, bias, x, g


def _check_resid_rows(resid, x0, X, W, bias, rows):
    """resid' = x0 + X W^T + bias against float64 on `rows`: the fp32 accumulation bound (K / 32 + 2) u sum |x w| + 2 u |value|."""
    K = X.shape[1]
    Xr = X[rows].double()
    want = x0[rows].double() + Xr @ W.double().t() + bias.double()
    S = Xr.abs() @ W.double().abs().t() + x0[rows].double().abs() + bias.double().abs()
    err = (resid[rows].double() - want).abs()
    assert (err <= (K // 32 + 4) * R.U32 * S).all(), (err / S).max().item()
    return (err / S).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['w4', 'pp64'])
@pytest.mark.parametrize('shape', PRODUCER_SHAPES)
def test_producer_fp32_stream(cuda, family, shape, monkeypatch):
    """kind 2 (out_proj / c_proj on the fp32 stream, LN = 2): resid' bit-equal to vg_gemm's residual epilogue of the same family on the same
    operands (the same expression (acc + bias) + resid), x16 == f16(resid') bit for bit, every (mean, m2) partial written and equal to
    float64 statistics of the kernel's own resid' columns; resid' against float64 on sampled rows."""
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    _set_family(monkeypatch, family)
    M, N, K = shape
    X, W, bias, x, g = _producer_operands(M, N, K, cuda)
    P = _cols()
    resid = x.clone()
    x16 = torch.full((M, N), float('nan'), dtype=torch.float16, device=cuda)
    stats = torch.full((M, N // P, 2), float('nan'), device=cuda)
    assert _ln(2, X, W, bias, None, stats, None, N, resid, x16, M, N, K) == VG_OK
    plain = x.clone()
    check(lib.vg_gemm(1, 2, ptr(X), ptr(W), ptr(bias), None, ptr(plain), M, N, K, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(resid, plain), (resid - plain).abs().max().item()
    e_mean, e_m2 = R.check_producer_f32(resid, x16, stats, P)
    rows = sample_rows(M, g).to(cuda) if M > 768 else torch.arange(M, device=cuda)
    e_r = _check_resid_rows(resid, x, X, W, bias, rows)
    print(f'producer fp32 {family} {shape}: mean {e_mean:.2e} of mean|v|, m2 {e_m2:.2e} rel, resid {e_r:.2e} of sum|.|')


@pytest.mark.gpu
@pytest.mark.parametrize('shape', PRODUCER_SHAPES)
def test_producer_fp16_pair(cuda, shape, monkeypatch):
    """kind 3 (EPI_BIAS_RESID_HL, k_gemm_f16_w4 only): the stream as a real pair hi = f16(x), lo = f16(x - hi); kind 2 on the same X, W,
    bias with resid = hi + lo (exact in fp32) gives v; then hi' == f16(v), lo' == f16(v - hi') bit for bit (the accumulator bits do not
    depend on the epilogue's layout: tests/test_gemm.py w4 == pp64), |lo'| <= ulp(hi') / 2, partials = float64 statistics of hi' + lo'."""
    _set_family(monkeypatch, 'w4')
    M, N, K = shape
    X, W, bias, x, g = _producer_operands(M, N, K, cuda)
    P = _cols()
    hi, lo = R.make_pair(x)
    v = hi.float() + lo.float()
    assert torch.equal((v.double() - hi.double() - lo.double()), torch.zeros_like(v, dtype=torch.float64))
    x16 = torch.empty(M, N, dtype=torch.float16, device=cuda)
    s2 = torch.full((M, N // P, 2), float('nan'), device=cuda)
    assert _ln(2, X, W, bias, None, s2, None, N, v, x16, M, N, K) == VG_OK
    hi2, lo2 = hi.clone(), lo.clone()
    stats = torch.full((M, N // P, 2), float('nan'), device=cuda)
    assert _ln(3, X, W, bias, None, stats, None, N, lo2, hi2, M, N, K) == VG_OK
    e_mean, e_m2 = R.check_pair(hi2, lo2, stats, v, P)
    moved = (lo2 != 0).float().mean().item()
    assert moved > 0.5, moved                           # (lo' carries bits: a zero lo' would pass the half-ulp test)
    print(f'producer pair w4 {shape}: mean {e_mean:.2e} of mean|v|, m2 {e_m2:.2e} rel; lo != 0 in {moved:.1%}')


# ------------------------------------------------------------------------------------------------------------------- consumer
CONSUMER_SHAPES = [(256, 256, 256), (256, 768, 256), (768, 256, 512), (512, 1536, 512), (512, 2304, 768), (256, 3072, 768),
                   (256, 3072, 1024), (256, 4096, 1024)]       # one tile, three tiles (both ways), in_proj / c_fc of widths 512, 768, 1024
LARGE_CONSUMER = [(64256, 2304, 768, 0), (65792, 768, 768, 1), (65792, 2304, 768, 1), (64256, 768, 768, 0)]


def _consumer_operands(M, N, K, P, cuda, gen):
    """fp32 rows x, LayerNorm g / beta, W, b -> the fold's inputs exactly as the tower builds them (k_ln_fold) and the partials of x."""
    x = R.ln_rows(M, K, gen)
    gam = 1.0 + 0.3 * torch.randn(K, generator=gen)
    beta = 0.2 * torch.randn(K, generator=gen)
    W32 = _weights(N, K, gen)
    b = 0.1 * torch.randn(N, generator=gen)
    Wf, c1, c2 = R.fold_ln(W32, gam, beta, b)
    parts = R.partial_stats(x.to(cuda), P).float()
    return [t.to(cuda) for t in (x, gam, beta, W32, b, Wf, c1, c2)] + [parts]


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['w4', 'pp64'])
@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('shape', CONSUMER_SHAPES)
def test_consumer(cuda, family, kind, shape, monkeypatch):
    """kinds 0 / 1 (in_proj / c_fc, LN = 1) on rows of very different statistics (gemm_ln_ref.ln_rows): (a) against the formula on its exact
    inputs (X16, W', c1, c2, the partials merged with P = vg_gemm_ln_partial_cols()), (b) against LayerNorm(x) W^T + b [QuickGELU] from fp32
    x, g, beta, W, b (bounds: gemm_ln_ref.consumer_formula / semantic_bound_extra)."""
    _set_family(monkeypatch, family)
    M, N, K = shape
    P = _cols()
    g = _gen('consumer', M, N, K, kind)
    x, gam, beta, W32, b, Wf, c1, c2, parts = _consumer_operands(M, N, K, P, cuda, g)
    X16 = x.half()
    C = torch.full((M, N), float('nan'), dtype=torch.float16, device=cuda)
    assert _ln(kind, X16, Wf, c2, c1, parts, C, N, None, None, M, N, K) == VG_OK
    e_a, frac, tight = R.check_consumer_formula(C, X16, Wf, c1, c2, parts, P, kind == 1)
    e_b = R.check_consumer_semantic(C, x, gam, beta, W32, b, X16, Wf, c1, c2, parts, P, kind == 1)
    print(f'consumer kind {kind} {family} {shape}: formula {e_a:.2f} ulp ({frac:.2%} exact of the {tight:.0%} well-conditioned), '
          f'LayerNorm reference {e_b:.2f} ulp')


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['w4', 'pp64'])
@pytest.mark.parametrize('shape', LARGE_CONSUMER)
def test_consumer_large_launches(cuda, family, shape, monkeypatch):
    """251 / 257 row tiles x 3 / 9 column tiles: every persistent w4 workgroup runs several tiles, each from the statistics, bias and c1
    prefetched during the previous one (issue_raw / take_raw).  The formula reference on sampled rows (sample_rows)."""
    _set_family(monkeypatch, family)
    M, N, K, kind = shape
    P = _cols()
    g = _gen('consumer-large', M, N, K, kind)
    x, gam, beta, W32, b, Wf, c1, c2, parts = _consumer_operands(M, N, K, P, cuda, g)
    X16 = x.half()
    C = torch.full((M, N), float('nan'), dtype=torch.float16, device=cuda)
    assert _ln(kind, X16, Wf, c2, c1, parts, C, N, None, None, M, N, K) == VG_OK
    assert torch.isfinite(C).all()
    rows = sample_rows(M, g).to(cuda)
    e_a, frac, tight = R.check_consumer_formula(C[rows], X16[rows], Wf, c1, c2, parts[rows], P, kind == 1)
    print(f'consumer kind {kind} {family} {shape}, {len(rows)} rows: formula {e_a:.2f} ulp ({frac:.2%} exact of the {tight:.0%} well-conditioned)')


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['w4', 'pp64'])
def test_consumer_strided_column_offset(cuda, family, monkeypatch):
    """The class-row in_proj's launch shape: C + W with row stride 3W + 64 and N = 2W; columns outside [W, 3W) stay untouched (NaN)."""
    _set_family(monkeypatch, family)
    M, Wd = 512, 768
    N, K, ldc = 2 * Wd, Wd, 3 * Wd + 64
    P = _cols()
    g = _gen('strided', family)
    x, gam, beta, W32, b, Wf, c1, c2, parts = _consumer_operands(M, N, K, P, cuda, g)
    X16 = x.half()
    C = torch.full((M, ldc), float('nan'), dtype=torch.float16, device=cuda)
    assert _ln(0, X16, Wf, c2, c1, parts, C, ldc, None, None, M, N, K, c_off=Wd) == VG_OK
    assert torch.isnan(C[:, :Wd]).all() and torch.isnan(C[:, 3 * Wd:]).all()
    e_a, frac, _ = R.check_consumer_formula(C[:, Wd:3 * Wd], X16, Wf, c1, c2, parts, P, False)
    print(f'consumer strided {family}: {e_a:.2f} ulp, {frac:.2%} exact')


# ------------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.gpu
@pytest.mark.parametrize('stream', ['fp32-w4', 'fp32-pp64', 'pair-w4'])
def test_producer_consumer_chain(cuda, stream, monkeypatch):
    """out_proj (producer: x' = x + h W_o^T + b_o, its fp16 copy and partials) -> c_fc with ln_2 folded (consumer, QuickGELU), as the block
    runs them, against the float64 block arithmetic QuickGELU(LayerNorm(x') W_fc^T + b_fc).  Bound: the semantic bound of the consumer on
    x', plus what the stream's own rounding (fp32, or 22 bits of the pair) moves through rstd |W'|."""
    kind_p = 3 if stream.startswith('pair') else 2
    _set_family(monkeypatch, stream.split('-')[1])
    P = _cols()
    M, Wd = 768, 768
    g = _gen('chain', stream)
    h = (torch.randn(M, Wd, generator=g) * 0.5).half().to(cuda)
    Wo = _weights(Wd, Wd, g).half().to(cuda)
    bo = (torch.randn(Wd, generator=g) * 0.1).to(cuda)
    x = R.ln_rows(M, Wd, g).to(cuda)
    gam = (1.0 + 0.3 * torch.randn(Wd, generator=g)).to(cuda)
    beta = (0.2 * torch.randn(Wd, generator=g)).to(cuda)
    Wfc = _weights(4 * Wd, Wd, g).to(cuda)
    bfc = (0.1 * torch.randn(4 * Wd, generator=g)).to(cuda)
    Wf, c1, c2 = R.fold_ln(Wfc, gam, beta, bfc)
    stats = torch.full((M, Wd // P, 2), float('nan'), device=cuda)
    if kind_p == 2:
        resid, x16 = x.clone(), torch.empty(M, Wd, dtype=torch.float16, device=cuda)
        x0 = x.double()
        assert _ln(2, h, Wo, bo, None, stats, None, Wd, resid, x16, M, Wd, Wd) == VG_OK
        stream_now = resid.double()
    else:
        x16, resid = R.make_pair(x)
        x0 = x16.double() + resid.double()
        assert _ln(3, h, Wo, bo, None, stats, None, Wd, resid, x16, M, Wd, Wd) == VG_OK
        stream_now = x16.double() + resid.double()
    xp = x0 + h.double() @ Wo.double().t() + bo.double()              # the block's float64 x'
    S = h.double().abs() @ Wo.double().abs().t() + x0.abs() + bo.double().abs()
    d_stream = (stream_now - xp).abs()
    assert (d_stream <= (Wd // 32 + 4) * R.U32 * S + (2.0 ** -22) * xp.abs() + 2.0 ** -24).all()
    C = torch.full((M, 4 * Wd), float('nan'), dtype=torch.float16, device=cuda)
    assert _ln(1, x16, Wf, c2, c1, stats, C, 4 * Wd, None, None, M, 4 * Wd, Wd) == VG_OK
    ln, rstd = R.layernorm64(xp, gam, beta)
    y = R.quick_gelu(ln @ Wfc.double().t() + bfc.double())
    _, pre = R.consumer_formula(x16, Wf, c1, c2, stats, P, True)
    extra = R.semantic_bound_extra(xp.float(), gam, Wfc, Wf, rstd)
    carry = rstd[:, None] * (d_stream @ Wf.double().abs().t())
    # the kernel's partials describe its own stream, not x': their merged (mean, rstd) against x''s
    stat = R.stats_deviation(stats, P, xp, ln @ Wfc.double().t() + bfc.double(), c1, c2) + R.U32 * c2.double().abs()[None, :]
    bound = R.ulp16(y) + pre + R.GELU_SLOPE * (extra + carry + stat)
    err = (C.double() - y).abs()
    assert torch.isfinite(C).all()
    assert (err <= bound).all(), ((err - bound).max().item(), (err > bound).nonzero()[0].tolist())
    print(f'chain {stream}: max |C - y| {(err / R.ulp16(y)).max().item():.2f} ulp, within {(err / bound).max().item():.2f} of the bound')


# ------------------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.gpu
def test_rejections(cuda, monkeypatch):
    """Launches the kernels cannot compute correctly return VG_ERR_ARG and write nothing: pp64 consumer with K = 1280 (it merges at most
    four 256-column partials), w4 consumer with K % 128 != 0, producers with ldc != N, the pair producer under VG_GEMM_W4=0."""
    M, N = 256, 512
    big = torch.zeros(M * 4096, dtype=torch.float16, device=cuda)
    f32 = torch.zeros(M * 4096, device=cuda)
    st = torch.zeros(M * 64, device=cuda)
    C = torch.full((M, 1024), float('nan'), dtype=torch.float16, device=cuda)
    monkeypatch.setenv('VG_GEMM_W4', '0')
    assert _ln(0, big, big, f32, f32, st, C, N, None, None, M, N, 1280) == VG_ERR_ARG
    assert _ln(1, big, big, f32, f32, st, C, N, None, None, M, N, 1280) == VG_ERR_ARG
    assert _ln(0, big, big, f32, f32, st, C, N, None, None, M, N, 1024) == VG_OK        # (the largest K it merges)
    C.fill_(float('nan'))
    assert _ln(2, big, big, f32, None, st, None, N + 64, f32, big, M, N, 512) == VG_ERR_ARG
    assert _ln(3, big, big, f32, None, st, None, N, f32, big, M, N, 512) == VG_ERR_ARG
    monkeypatch.setenv('VG_GEMM_W4', '1')
    assert _ln(0, big, big, f32, f32, st, C, N, None, None, M, N, 320) == VG_ERR_ARG
    assert _ln(0, big, big, f32, f32, st, C, N, None, None, M, N, 1280) == VG_ERR_ARG
    assert _ln(2, big, big, f32, None, st, None, N + 64, f32, big, M, N, 512) == VG_ERR_ARG
    assert _ln(3, big, big, f32, None, st, None, N + 64, f32, big, M, N, 512) == VG_ERR_ARG
    assert _ln(0, big, big, f32, f32, st, C, N - 8, None, None, M, N, 512) == VG_ERR_ARG     # ldc < N
    assert _ln(4, big, big, f32, f32, st, C, N, f32, big, M, N, 512) == VG_ERR_ARG
    assert torch.isnan(C).all()


# ------------------------------------------------------------------------------------------------------------------- the checkers (CPU)
def test_checkers_reject_synthesised_faults():
    """The checkers above have teeth: outputs synthesised from the formulas pass them, and the same outputs with (i) two rows' statistics
    swapped, (ii) a merge with P = 256 where 128 is right, (iii) lo' = 0 are rejected -- without running a broken kernel."""
    g = torch.Generator().manual_seed(11)
    M, N, K, P = 256, 512, 768, 128
    x, gam, beta, W32, b, Wf, c1, c2, parts = _consumer_operands(M, N, K, P, torch.device('cpu'), g)
    X16 = x.half()
    for gelu in (False, True):
        y, _ = R.consumer_formula(X16, Wf, c1, c2, parts, P, gelu)
        C = y.half()
        R.check_consumer_formula(C, X16, Wf, c1, c2, parts, P, gelu)
        R.check_consumer_semantic(C, x, gam, beta, W32, b, X16, Wf, c1, c2, parts, P, gelu)
        swapped = parts.clone()
        swapped[[7, 200]] = parts[[200, 7]]
        with pytest.raises(AssertionError):                                       # (i)
            R.check_consumer_formula(C, X16, Wf, c1, c2, swapped, P, gelu)
        Cw = R.consumer_formula(X16, Wf, c1, c2, parts, P, gelu, factor=256)[0].half()
        with pytest.raises(AssertionError):                                       # (ii)
            R.check_consumer_formula(Cw, X16, Wf, c1, c2, parts, P, gelu)
        with pytest.raises(AssertionError):
            R.check_consumer_semantic(Cw, x, gam, beta, W32, b, X16, Wf, c1, c2, parts, P, gelu)
    # producers: the fp32 stream and the pair, synthesised from their definitions
    v = R.ln_rows(M, N, g) + torch.randn(M, N, generator=g)
    stats = R.partial_stats(v, P).float()
    R.check_producer_f32(v, v.half(), stats, P)
    sw = stats.clone()
    sw[[3, 100]] = stats[[100, 3]]
    with pytest.raises(AssertionError):                                           # (i)
        R.check_producer_f32(v, v.half(), sw, P)
    with pytest.raises(AssertionError):                                           # (ii): 256-column partials laid out as 128-column ones
        R.check_partials(R.partial_stats(v, 256).float().repeat_interleave(2, 1), v, P)
    hi, lo = R.make_pair(v)
    pstats = R.partial_stats(hi.float() + lo.float(), P).float()
    R.check_pair(hi, lo, pstats, v, P)
    with pytest.raises(AssertionError):                                           # (iii)
        R.check_pair(hi, torch.zeros_like(lo), pstats, v, P)
    with pytest.raises(AssertionError):
        R.check_pair(hi, lo, sw, v, P)
    nan = stats.clone()
    nan[5, 1] = float('nan')
    with pytest.raises(AssertionError):                                           # an unwritten partial
        R.check_partials(nan, v, P)
