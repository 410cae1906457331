"""Plain float64 references and checkers of the folded-LayerNorm GEMM epilogues (vg_gemm_ln; csrc/vit.hip k_gemm_f16_w4 / k_gemm_f16_pp64
LN = 1 / 2, EPI_BIAS_RESID_HL), shared by tests/test_gemm_ln.py and its CPU test of the checkers themselves.

Every checker raises AssertionError on a mismatch and returns the largest deviation it measured (for the test log).  They work on torch
tensors on any device; the arithmetic of the references is float64 throughout.

Notation: P = columns per partial statistic (128 for k_gemm_f16_w4, 256 for k_gemm_f16_pp64), a partial is (mean, m2) of P consecutive
columns of a row, m2 = the sum of squared deviations from that mean."""
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
EPS = 1e-5                # LayerNorm epsilon (model.py's nn.LayerNorm default)
GELU_SLOPE = 1.13         # max |d/dx x sigmoid(1.702 x)| (1.129 at x = 2.4): an error before QuickGELU grows at most by this


def ulp16(v):
    """Spacing of fp16 numbers at |v| (float64), subnormals included: 2^(e - 10) for |v| in [2^e, 2^(e+1)), at least 2^-24."""
    v = v.double()
    e = ((v.view(torch.int64) >> 52) & 0x7FF) - 1023            # floor(log2 |v|) from the exponent field (exact; 0 -> -1023)
    return ((torch.clamp(e, min=-14) - 10 + 1023) << 52).view(torch.float64)


def partial_stats(v, P):
    """(mean, m2) per row and P-column group of v [M, N] -> float64 [M, N / P, 2]."""
    M, N = v.shape
    g = v.double().reshape(M, N // P, P)
    mean = g.mean(-1)
    return torch.stack([mean, ((g - mean[..., None]) ** 2).sum(-1)], -1)


def merge_stats(parts, K, P, factor=None):
    """The consumer's merge of a row's K / P partials (Chan et al.) -> (mean, rstd) float64 [M]:
    mean = mean of the partial means, var = (sum m2 + P sum (mean_i - mean)^2) / K, rstd = 1 / sqrt(var + 1e-5).
    (`factor` replaces that P: only to synthesise the output of a kernel that merges with the wrong granularity.)"""
    parts = parts.double()
    assert parts.shape[1] * P == K, (parts.shape, K, P)
    means, m2 = parts[..., 0], parts[..., 1]
    mean = means.mean(-1)
    var = (m2.sum(-1) + (P if factor is None else factor) * ((means - mean[:, None]) ** 2).sum(-1)) / K
    return mean, 1.0 / torch.sqrt(var + EPS)


def quick_gelu(y):
    return y * torch.sigmoid(1.702 * y)


def gelu_slope(y, r):
    """A bound of |QuickGELU'| on [y - r, y + r] (r small): its largest value at the ends and the middle plus 0.01 (|QuickGELU''| <= 0.9:
    the slope moves by at most 0.9 r inside, and r is below 0.01 wherever the slope is not already bounded by GELU_SLOPE)."""
    def d(t):
        s = torch.sigmoid(1.702 * t)
        return (s + 1.702 * t * s * (1 - s)).abs()
    return torch.minimum(torch.maximum(torch.maximum(d(y - r), d(y + r)), d(y)) + 0.01 + 0.9 * r, torch.full_like(y, GELU_SLOPE))


def fold_ln(W32, g, beta, b):
    """The folded weights exactly as k_ln_fold builds them (csrc/vit.hip): W' = f16(fp32(g[k] W[n,k])), c1[n] = fp32(sum_k W'[n,k]) over the
    ROUNDED weights, c2[n] = fp32(b[n] + sum_k beta[k] W[n,k]) (sums in float64)."""
    Wf = (g.float()[None, :] * W32.float()).half()
    c1 = Wf.double().sum(1).float()
    c2 = (b.double() + W32.double() @ beta.double()).float()
    return Wf, c1, c2


# ---------------------------------------------------------------------------------------------- consumer (kinds 0 / 1)
def consumer_formula(X16, Wf, c1, c2, parts, P, gelu, factor=None):
    """float64 value of the consumer's formula on its exact inputs, and the bound of what fp32 arithmetic may add to it (before the final fp16
    rounding).  -> (y [M, N] float64, pre_bound [M, N] float64).

    pre_bound, per element, in the order the kernel computes y = rstd (acc - mean c1) + c2:
      acc:         the fp32 accumulation of K exact fp16 products in K / 32 MFMA steps: (K / 32 + 2) u sum_k |x_k w_k|
      mean:        the fp32 sum and division of the K / P partial means: (K / P + 2) u max |mean_i|, times |c1|
      mean * c1 (and c1 held in fp32), the subtraction, rstd (fp32 merge + rsqrt: 64 u relative), times rstd, the + c2: one u each of their magnitudes
      QuickGELU:   the error above times the slope bound on its interval (gelu_slope), plus the exp2 / rcp approximations (4 u relative)
    The terms in acc and mean grow with |mean| / std of the row (rstd multiplies values of size |mean| |c1|): the folded form subtracts
    two large, nearly equal numbers there, which a separate LayerNorm would not.  The bound grows with it per row instead of loosening
    every row."""
    K = X16.shape[1]
    X, W = X16.double(), Wf.double()
    acc = X @ W.t()
    S = X.abs() @ W.abs().t()
    mean, rstd = merge_stats(parts, K, P, factor)
    mc = mean[:, None] * c1.double()[None, :]
    core = acc - mc
    y = rstd[:, None] * core + c2.double()[None, :]
    d_mean = (K // P + 2) * U32 * parts.double()[..., 0].abs().amax(-1)
    e_core = (K // 32 + 2) * U32 * S + d_mean[:, None] * c1.double().abs()[None, :] + U32 * (2 * mc.abs() + acc.abs() + core.abs())
    pre = rstd[:, None] * e_core + 64 * U32 * (rstd[:, None] * core).abs() + U32 * y.abs()
    if gelu:
        pre = gelu_slope(y, pre) * pre
        y = quick_gelu(y)
        pre = pre + 4 * U32 * y.abs()
    return y, pre


def check_consumer_formula(C, X16, Wf, c1, c2, parts, P, gelu, min_exact=0.99):
    """C (the kernel's fp16 output) against consumer_formula: every element within one fp16 ulp + pre_bound; of the elements whose
    pre_bound is below a quarter ulp (fp32 arithmetic cannot move them across a rounding boundary but by chance), at least `min_exact`
    equal to the correctly rounded reference.  -> (max |C - y| / ulp16(y), fraction exact, fraction of such elements)"""
    y, pre = consumer_formula(X16, Wf, c1, c2, parts, P, gelu)
    got = C.double()
    assert torch.isfinite(got).all(), 'non-finite outputs (unwritten rows?)'
    ulp = ulp16(y)
    err = (got - y).abs()
    bad = err > ulp + pre
    assert not bad.any(), f'{int(bad.sum())} elements out of bound; worst {(err - ulp - pre).max().item():.3e} beyond, at {bad.nonzero()[0].tolist()}'
    tight = pre < 0.25 * ulp
    exact = (got == y.half().double()) & tight
    frac = exact.sum().item() / max(1, tight.sum().item())
    assert tight.float().mean().item() > 0.5, tight.float().mean().item()
    assert frac >= min_exact, frac
    return (err / ulp).max().item(), frac, tight.float().mean().item()


def semantic_bound_extra(x, g, W32, Wf, rstd):
    """What the fold's roundings add on top of consumer_formula's bound when C is compared with LayerNorm(x) W^T + b from fp32 x:
    the fp16 rounding of x (<= ulp16(x) / 2 each, times |W'|) and of W' = f16(fp32(g W)) (<= ulp16(g W) / 2 + u |g W| each, times
    |x - mean|), both times rstd.  The first is the folded form's precision loss: it scales with |x| / std, i.e. with |mean| / std and with
    outliers."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    gw = (g.double()[None, :] * W32.double()).abs()
    e_x = (ulp16(x.double()) / 2) @ Wf.double().abs().t()
    e_w = (xd - mean).abs() @ (ulp16(gw) / 2 + U32 * gw).t()
    return rstd[:, None] * (e_x + e_w)


def layernorm64(x, g, beta):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + EPS) * g.double() + beta.double(), (1.0 / torch.sqrt(var + EPS))[:, 0]


def stats_deviation(parts, P, x, y_lin, c1, c2):
    """What the partials' own deviation from x's exact statistics (fp32 rounding of the partials, or of the stream they describe) moves
    y_lin = LayerNorm(x) W^T + b by: rstd |mean_parts - mean_x| |c1| + |rstd_parts / rstd_x - 1| |y_lin - c2| (measured, per element)."""
    K = x.shape[1]
    mean_k, rstd_k = merge_stats(parts, K, P)
    xd = x.double()
    _, rstd_x = layernorm64(xd, torch.ones(K, dtype=torch.float64, device=x.device), torch.zeros(K, dtype=torch.float64, device=x.device))
    return rstd_k[:, None] * (mean_k - xd.mean(1)).abs()[:, None] * c1.double().abs()[None, :] + \
        (rstd_k / rstd_x - 1).abs()[:, None] * (y_lin - c2.double()[None, :]).abs()


def check_consumer_semantic(C, x, g, beta, W32, b, X16, Wf, c1, c2, parts, P, gelu):
    """C against the operation the fold stands for, y = [QuickGELU](LayerNorm(x) W^T + b) in float64 from fp32 x, g, beta, W, b:
    |C - y| <= ulp16(y) + consumer_formula's pre_bound + slope * (semantic_bound_extra + stats_deviation + u |c2|).
    -> max |C - y| / ulp16(y)"""
    ln, rstd = layernorm64(x, g, beta)
    y = ln @ W32.double().t() + b.double()
    extra = semantic_bound_extra(x, g, W32, Wf, rstd) + stats_deviation(parts, P, x, y, c1, c2) + U32 * c2.double().abs()[None, :]
    if gelu:
        y = quick_gelu(y)
        extra = extra * GELU_SLOPE
    _, pre = consumer_formula(X16, Wf, c1, c2, parts, P, gelu)
    ulp = ulp16(y)
    err = (C.double() - y).abs()
    bad = err > ulp + pre + extra
    assert not bad.any(), f'{int(bad.sum())} elements out of bound; worst {(err - ulp - pre - extra).max().item():.3e} beyond, at {bad.nonzero()[0].tolist()}'
    return (err / ulp).max().item()


# ---------------------------------------------------------------------------------------------- producers (kinds 2 / 3)
def check_partials(stats, v, P):
    """The kernel's partials [M, N / P] (float pairs) against float64 statistics of v [M, N] (the values they describe): every partial
    written (the buffer was pre-filled with NaN), mean within 2e-6 mean|v| of the group, m2 within 1e-5 relative (+ the P delta^2 an fp32
    mean that is off by 2e-6 mean|v| adds).  -> (max mean error / mean|v|, max relative m2 error)"""
    M, N = v.shape
    stats = stats.reshape(M, -1, 2).double()
    assert stats.shape[1] * P == N, (stats.shape, N, P)
    assert torch.isfinite(stats).all(), f'{int((~torch.isfinite(stats)).sum())} partials unwritten'
    want = partial_stats(v, P)
    mabs = v.double().abs().reshape(M, N // P, P).mean(-1)
    e_mean = (stats[..., 0] - want[..., 0]).abs()
    e_m2 = (stats[..., 1] - want[..., 1]).abs()
    tol_m2 = 1e-5 * want[..., 1] + P * (2e-6 * mabs) ** 2
    assert (e_mean <= 2e-6 * mabs + 1e-30).all(), (e_mean / (mabs + 1e-30)).max().item()
    assert (e_m2 <= tol_m2).all(), ((e_m2 - tol_m2) / (want[..., 1] + 1e-30)).max().item()
    return (e_mean / (mabs + 1e-30)).max().item(), (e_m2 / (want[..., 1] + 1e-30)).max().item()


def check_producer_f32(resid, x16, stats, P):
    """kind 2's outputs among themselves: x16 is the fp16 copy of the new stream bit for bit, the partials are its statistics."""
    assert torch.equal(x16, resid.half()), 'x16 != f16(resid)'
    return check_partials(stats, resid, P)


def check_pair(hi, lo, stats, v32, P):
    """kind 3's outputs against v32, the fp32 stream kind 2 computes from the same operands with resid = hi_in + lo_in (exact in fp32):
    hi' == f16(v32) and lo' == f16(v32 - hi') bit for bit (the same fp32 expression (acc + bias) + (hi + lo) in both epilogues),
    |lo'| <= ulp16(hi') / 2, and the partials are the statistics of hi' + lo'."""
    want_hi = v32.half()
    want_lo = (v32 - want_hi.float()).half()
    assert torch.equal(hi, want_hi), f'hi: {int((hi != want_hi).sum())} differ'
    assert torch.equal(lo, want_lo), f'lo: {int((lo != want_lo).sum())} differ'
    assert (lo.double().abs() <= ulp16(hi) / 2).all(), 'lo beyond half an ulp of hi'
    return check_partials(stats, hi.float() + lo.float(), P)


def make_pair(x):
    """An fp32 stream as an fp16 pair: hi = f16(x), lo = f16(x - hi)."""
    hi = x.half()
    return hi, (x - hi.float()).half()


def ln_rows(M, K, gen, outliers=(3, 77), constant_row=5):
    """Residual-stream-like rows with very different statistics (a row <-> statistic mix-up must fail loudly): per-row mean from -5 to 5,
    scale log-uniform in [0.01, 50], a few CLIP-like outlier columns (+-100) in most rows, and one constant row (variance 0: rstd =
    1 / sqrt(1e-5)).  float32 [M, K]."""
    mean = torch.rand(M, 1, generator=gen, dtype=torch.float64) * 10 - 5
    scale = torch.exp(torch.rand(M, 1, generator=gen, dtype=torch.float64) * (torch.log(torch.tensor(5000.0))) + torch.log(torch.tensor(0.01)))
    x = mean + scale * torch.randn(M, K, generator=gen, dtype=torch.float64)
    sgn = torch.where(torch.rand(M, generator=gen) < 0.5, -1.0, 1.0).double()
    has = torch.rand(M, generator=gen) < 0.7
    for c in outliers:
        if c < K:
            x[has, c] = 100.0 * sgn[has]
    x[constant_row % M] = 3.0
    return x.float()
