"""Plain float64 references, error bounds, input families and checkers of the projection GEMM's plain epilogues (vg_gemm; csrc/vit.hip
k_gemm_f16, k_gemm_f16_pp64, k_gemm_f16_w4, k_gemm_f32, k_gemm_f32_mfma), shared by tests/test_gemm_families.py, tests/test_gemm.py and
the CPU test of the checkers themselves.  The shared pieces (U32, ulp16, quick_gelu, gelu_slope) are those of gemm_ln_ref.

Every checker raises AssertionError on a mismatch and returns what it measured (for the test log).  They work on torch tensors on any
device; the arithmetic of the references is float64 throughout, from the exact bits the kernel reads.

Epilogues (vilgod_hip.h vg_gemm):  0: X W^T + b   1: QuickGELU of that   2: resid + (X W^T + b)   3: X W^T   4: f16(resid16 + f16(X W^T + b))

Bound of a correct kernel's deviation BEFORE the rounding of the output, with S = |X| |W|^T + |b| (+ |resid|):
    (c + 2) u S  +  u |value| per further fp32 operation of the epilogue,       u = 2^-24
c = the number of dependent fp32 additions into one accumulator: K / 32 for k_gemm_f16_pp64 and k_gemm_f16_w4 (16 x 16 x 32 MFMA), K / 16
for k_gemm_f16 (32 x 32 x 16), K for the two fp32 kernels (one fmaf chain over ascending k).  Epilogue 1: that bound times the slope of
QuickGELU on its interval plus 4 u |y| for exp2 / rcp (the term of gemm_ln_ref.consumer_formula).  None of these is tuned on a GPU."""
import zlib

import torch

from gemm_ln_ref import U32, ulp16, quick_gelu, gelu_slope

FAMILY_CODES = {'f16': 0, 'pp64': 1, 'w4': 2, 'f32': 3, 'f32_mfma': 4}       # vg_gemm_family's codes
MFMA_K = {'f16': 16, 'pp64': 32, 'w4': 32, 'f32': 1, 'f32_mfma': 1}          # K elements per dependent fp32 addition
KTILE = {'f16': 32, 'pp64': 64, 'w4': 64, 'f32': 16, 'f32_mfma': 16}         # K elements per pipeline step (the synthesised faults use it)
KINDS = ('gauss', 'integer', 'onehot')
EXACT_MAX_K = 768          # the exactness clause of fp16 outputs holds up to here (beyond, too few elements have a bound below ulp / 4)


def family_dtype(family):
    return 0 if family.startswith('f32') else 1


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def round16(v):
    """float64 -> the nearest fp16 value (ties to even), as float64, in ONE rounding (torch's double -> half goes through float)."""
    u = ulp16(v)
    return torch.round(v.double() / u) * u


def trunc16(v):
    """float64 -> the fp16 value next to it toward zero (only to synthesise a kernel that truncates)."""
    u = ulp16(v)
    return torch.trunc(v.double() / u) * u


# ---------------------------------------------------------------------------------------------------------------------- inputs
class Operands:
    """One case's operands, as the kernel reads them: X [M, K], W [N, K] in the compute dtype, bias fp32 [N], resid fp32 [M, N] (epilogue
    2), resid16 fp16 [M, N] (epilogue 4).  `products()` caches X W^T and |X| |W|^T in float64 for every epilogue of the case."""

    def __init__(self, kind, X, W, bias, resid, resid16, onehot_k=None):
        self.kind, self.X, self.W, self.bias, self.resid, self.resid16, self.onehot_k = kind, X, W, bias, resid, resid16, onehot_k
        self._prod = None

    @property
    def shape(self):
        return self.X.shape[0], self.W.shape[0], self.X.shape[1]

    def products(self):
        if self._prod is None:
            if self.onehot_k is not None:             # one product per output: W[n, k(m)]
                acc = self.W.double()[:, self.onehot_k].t().contiguous()
                self._prod = (acc, acc.abs())
            else:
                X, W = self.X.double(), self.W.double()
                self._prod = (X @ W.t(), X.abs() @ W.abs().t())
        return self._prod

    def to(self, device):
        o = Operands(self.kind, self.X.to(device), self.W.to(device), self.bias.to(device), self.resid.to(device),
                     self.resid16.to(device), None if self.onehot_k is None else self.onehot_k.to(device))
        return o

    def rows(self, rows):
        """The case restricted to some rows of X (sampled rows of a large launch)."""
        return Operands(self.kind, self.X[rows], self.W, self.bias, self.resid[rows], self.resid16[rows],
                        None if self.onehot_k is None else self.onehot_k[rows])


def onehot_params(M, K):
    """(a, s) of the onehot family for a shape: a = 1 with every shift s = 0, M, 2 M, ... < K (rows 0 .. M - 1 then name the columns
    s .. s + M - 1: together EVERY k), and a = 65 (consecutive rows walk the slots of a 64-wide K-tile and step one K-tile on)."""
    return [(1, s) for s in range(0, K, M)] + [(65, 3)]


def operands(kind, M, N, K, dtype, a=1, s=0):
    """Seeded operands of one input family (`dtype` 1: fp16 X and W, 0: fp32).
    gauss:   X ~ 0.5 N(0,1), W ~ 0.05 N(0,1) with a ramp on column 0 (asymmetric: a transposed tile must not pass), b ~ 0.1 N(0,1)
    integer: X, W integers in [-4, 4], b and resid integers in [-8, 8]: every partial sum is an integer below 2^24 for K <= 3072, so the
             fp32 result is exact in ANY accumulation order
    onehot:  X[m, (a m + s) mod K] = 1, W[n, k] = ((131 n + 17 k) mod 127) - 63, integer b: output (m, n) names one (n, k)"""
    g = gen(kind, M, N, K, dtype, a, s)
    td = torch.float16 if dtype == 1 else torch.float32
    k_of = None
    if kind == 'gauss':
        X = torch.randn(M, K, generator=g) * 0.5
        W = torch.randn(N, K, generator=g) * 0.05
        W[:, 0] += torch.arange(N) * 1e-3
        bias = torch.randn(N, generator=g) * 0.1
        resid = torch.randn(M, N, generator=g)
        resid16 = (torch.randn(M, N, generator=g) * 2).half()
    else:
        def ints(lo, hi, *shape):
            return torch.randint(lo, hi + 1, shape, generator=g).float()
        bias, resid = ints(-8, 8, N), ints(-8, 8, M, N)
        resid16 = ints(-8, 8, M, N).half()
        if kind == 'integer':
            X, W = ints(-4, 4, M, K), ints(-4, 4, N, K)
        else:
            assert kind == 'onehot', kind
            k_of = (a * torch.arange(M) + s) % K
            X = torch.zeros(M, K)
            X[torch.arange(M), k_of] = 1.0
            W = (((131 * torch.arange(N)[:, None] + 17 * torch.arange(K)[None, :]) % 127) - 63).float()
    return Operands(kind, X.to(td), W.to(td), bias, resid, resid16, k_of)


# ---------------------------------------------------------------------------------------------------------------------- reference
def formula(o, epi, family):
    """float64 value of epilogue `epi` on the operands (before the rounding of the output; epilogue 4: of the projection X W^T + b before
    ITS rounding) and the bound of what a correct kernel of `family` may add to it.  -> (y, pre) float64 [M, N]"""
    K = o.X.shape[1]
    acc, S = o.products()
    c = K // MFMA_K[family]
    b = o.bias.double()[None, :]
    if epi == 3:
        return acc, (c + 2) * U32 * S
    y = acc + b
    S = S + b.abs()
    if epi == 2:
        r = o.resid.double()
        # two further additions: (acc + b) + resid in the 256 x 256 kernels and the fp32 kernels, acc + (b + resid) in k_gemm_f16
        out = y + r
        return out, (c + 2) * U32 * (S + r.abs()) + U32 * torch.maximum(y.abs(), (b + r).abs()) + U32 * out.abs()
    pre = (c + 2) * U32 * S + U32 * y.abs()
    if epi == 1:
        pre = gelu_slope(y, pre) * pre
        y = quick_gelu(y)
        pre = pre + 4 * U32 * y.abs()
    return y, pre


def reference_out(o, epi):
    """The correctly rounded output of the epilogue (what an exact kernel stores), float64."""
    y, _ = formula(o, epi, 'f32')
    if epi == 4:
        return round16(o.resid16.double() + round16(y))
    return round16(y) if (o.X.dtype == torch.float16 and epi in (0, 1)) else y


# ---------------------------------------------------------------------------------------------------------------------- checkers
def _where(bad):
    return bad.nonzero()[0].tolist()


def _finite(got):
    assert torch.isfinite(got).all(), f'{int((~torch.isfinite(got)).sum())} non-finite outputs (unwritten?), first at {_where(~torch.isfinite(got))}'


def check_bounded(got, y, pre, f16_out, exact_clause, min_exact=0.99):
    """The rule of gemm_ln_ref.check_consumer_formula.  fp16 outputs: every element within ulp16(y) + pre; with `exact_clause`, more than half
    of the elements have pre < ulp16(y) / 4 and at least `min_exact` of those equal the correctly rounded reference.  fp32 outputs: every
    element within pre.  -> (worst err / bound, fraction exact or None, share of qualifying elements or None)"""
    got = got.double()
    _finite(got)
    err = (got - y).abs()
    ulp = ulp16(y)
    bound = pre + ulp if f16_out else pre
    bad = err > bound
    assert not bad.any(), f'{int(bad.sum())} elements out of bound; worst {(err / bound).max().item():.3f} of it, first at {_where(bad)}'
    ratio = (err / bound).max().item()
    if not f16_out:
        return ratio, None, None
    tight = pre < 0.25 * ulp
    share = tight.double().mean().item()
    frac = ((got == round16(y)) & tight).sum().item() / max(1, int(tight.sum()))
    if exact_clause:
        assert share > 0.5, f'only {share:.3f} of the elements have a bound below a quarter ulp'
        assert frac >= min_exact, f'only {frac:.4f} of the elements with a bound below a quarter ulp are correctly rounded'
    return ratio, frac, share


def check_exact(got, want):
    """Bit for bit (the values are finite: equality of the numbers is equality of the bits, up to the sign of zero)."""
    got = got.double()
    _finite(got)
    bad = got != want
    assert not bad.any(), f'{int(bad.sum())} elements differ from the exact result; largest difference {(got - want).abs().max().item():.3e}, first at {_where(bad)}'
    return 0.0, 1.0, 1.0


def check_exact_gelu(got, y_lin):
    """Epilogue 1 on exact sums (integer, onehot): within the QuickGELU term 4 u |y| plus one fp16 ulp of y = QuickGELU(y_lin)."""
    got = got.double()
    _finite(got)
    y = quick_gelu(y_lin)
    err = (got - y).abs()
    bound = 4 * U32 * y.abs() + ulp16(y)
    bad = err > bound
    assert not bad.any(), f'{int(bad.sum())} elements out of bound; worst {(err / bound).max().item():.3f} of it, first at {_where(bad)}'
    return (err / bound).max().item(), None, None


def check_resid16(got, p, pre, resid16, min_exact=None):
    """Epilogue 4, resid' = f16(resid + f16(p32)) with p32 the kernel's fp32 projection, |p32 - p| <= pre: both roundings are monotone
    and the fp32 sum of two fp16 numbers rounds to fp16 like their exact sum (11 significant bits each: the fp32 rounding cannot create
    a tie), so resid' lies between f16(resid + f16(p - pre)) and f16(resid + f16(p + pre)), ends included -- per element, from the
    float64 product.  Where the two ends agree the element is determined bit for bit.
    -> (largest distance from f16(resid + f16(p)) in units of ulp16(p) + ulp16(it): at most 1, fraction equal to it, share of determined
    elements)"""
    got = got.double()
    _finite(got)
    r = resid16.double()
    lo, hi, mid = round16(r + round16(p - pre)), round16(r + round16(p + pre)), round16(r + round16(p))
    bad = (got < lo) | (got > hi)
    assert not bad.any(), f'{int(bad.sum())} elements outside [f16(r + f16(p - e)), f16(r + f16(p + e))], first at {_where(bad)}'
    frac = (got == mid).double().mean().item()
    if min_exact is not None:
        assert frac >= min_exact, frac
    return ((got - mid).abs() / (ulp16(p) + ulp16(mid))).max().item(), frac, (lo == hi).double().mean().item()


def check_case(got, o, epi, family):
    """The output of one launch (C, or resid for epilogues 2 and 4) against the case's reference, by the rule of its input family.
    -> (worst err / bound, fraction exact, qualifying share); the last two None where the rule has no such clause."""
    K = o.X.shape[1]
    y, pre = formula(o, epi, family)
    f16_out = o.X.dtype == torch.float16 and epi in (0, 1)
    if o.kind == 'gauss':
        if epi == 4:
            return check_resid16(got, y, pre, o.resid16, min_exact=0.9)        # (0.9: the clause of test_gemm_fp16_residual_epilogue)
        return check_bounded(got, y, pre, f16_out, exact_clause=f16_out and K <= EXACT_MAX_K)
    assert K <= 3072, 'the exact families need every partial sum below 2^24'
    if epi == 1:
        return check_exact_gelu(got, formula(o, 0, family)[0])
    return check_exact(got, reference_out(o, epi))


# ---------------------------------------------------------------------------------------------------------------------- guards
GUARD_ROWS = 256


def _bits(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def all_nan_fill(t):
    """Every element of t still holds the bits torch.full(..., nan) wrote."""
    return bool((_bits(t) == _bits(torch.full((1,), float('nan'), dtype=t.dtype, device=t.device))).all())


class Guarded:
    """A tensor as a view inside a larger allocation filled with NaN: GUARD_ROWS rows of its row length (vectors: GUARD_ROWS * 16 elements)
    before and after.  `intact()`: every guard byte still holds the fill pattern."""

    def __init__(self, t, device):
        row = t.shape[-1] if t.dim() > 1 else 16
        self.pad = GUARD_ROWS * row
        self.buf = torch.full((2 * self.pad + t.numel(),), float('nan'), dtype=t.dtype, device=device)
        self.fill = self.buf[:1].clone()
        self.view = self.buf[self.pad:self.pad + t.numel()].view(t.shape)
        self.view.copy_(t)

    def intact(self):
        want = _bits(self.fill)
        return bool((_bits(self.buf[:self.pad]) == want).all() and (_bits(self.buf[-self.pad:]) == want).all())


# ---------------------------------------------------------------------------------------------------------------------- emulation
FAULTS = ('drop_k', 'fp16_tile', 'trunc', 'bias_shift', 'swap_runs', 'swap_rows', 'gelu17', 'resid_twice', 'unwritten')
QGELU_C = (torch.tensor(-1.702, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)).item()


def emulate(o, epi, family, fault=None):
    """A float32 emulation of a correct kernel of `family` on the CPU -- the accumulator rounded to fp32 after every MFMA step (every
    fmaf for the fp32 kernels), the epilogue's operations in fp32 in the kernel's order, the output rounded once -- or, with `fault`, of
    a kernel with one synthesised fault:
      drop_k       the last K element of one K-tile dropped (rows of one 64-row group)
      fp16_tile    the last K-tile accumulated in fp16
      trunc        fp16 outputs truncated toward zero instead of rounded
      bias_shift   bias taken four columns further on
      swap_runs    a 4-wide column run swapped with its neighbour
      swap_rows    two rows of one 64-row group swapped
      gelu17       QuickGELU with 1.7
      resid_twice  the residual added twice in one tile
      unwritten    one tile left unwritten (NaN, the tests' prefill)
    -> the output as the kernel stores it (fp16 or fp32 tensor)."""
    M, N, K = o.shape
    step, kt = MFMA_K[family], KTILE[family]
    f16_in = o.X.dtype == torch.float16
    X = o.X.double().clone()
    W = o.W.double()
    r0 = 64 if M >= 128 else 32
    if fault == 'drop_k':
        X[r0:r0 + min(64, M - r0), (min(1, K // kt - 1) + 1) * kt - 1] = 0.0
    acc = torch.zeros(M, N, dtype=torch.float32)
    for k0 in range(0, K, step):
        acc = (acc.double() + X[:, k0:k0 + step] @ W[:, k0:k0 + step].t()).float()
        if fault == 'fp16_tile' and k0 >= K - kt:
            acc = acc.half().float()
    bias = o.bias.roll(-4) if fault == 'bias_shift' else o.bias
    tile = (slice(0, 64), slice(0, 64))
    if epi == 3:
        out = acc
    elif epi == 2:
        r = o.resid.clone()
        if fault == 'resid_twice':
            r[tile] = r[tile] * 2
        out = acc + (bias[None, :] + r) if family == 'f16' else (acc + bias[None, :]) + r
    else:
        v = acc + bias[None, :]
        if epi == 1:
            if f16_in:
                c = torch.tensor(QGELU_C if fault != 'gelu17' else QGELU_C * 1.7 / 1.702, dtype=torch.float32)
                v = v * (1.0 / (1.0 + torch.exp2(v * c)))
            else:
                v = v / (1.0 + torch.exp(torch.tensor(-1.702 if fault != 'gelu17' else -1.7, dtype=torch.float32) * v))
        if f16_in:
            v = trunc16(v).half() if fault == 'trunc' else v.half()
        if epi == 4:
            r = o.resid16.float()
            s = r + v.float()
            if fault == 'resid_twice':
                s[tile] = s[tile] + r[tile]
            v = trunc16(s).half() if fault == 'trunc' else s.half()
        out = v
    out = out.clone()
    if fault == 'swap_runs':
        out[:, [8, 9, 10, 11, 12, 13, 14, 15]] = out[:, [12, 13, 14, 15, 8, 9, 10, 11]]
    if fault == 'swap_rows':
        out[[r0 + 5, r0 + 21]] = out[[r0 + 21, r0 + 5]]
    if fault == 'unwritten':
        out[tile] = float('nan')
    return out
