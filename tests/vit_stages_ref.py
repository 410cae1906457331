"""Float64 references, derived error bounds, float32 emulations and fault generators of the image tower's small kernels (csrc/vit.hip:
k_im2col, k_embed_lnpre, k_layernorm, k_head, k_conv1_fold), shared by tests/test_vit_stages.py's GPU tests and its CPU test of the
checkers themselves.  numpy throughout; the references compute in float64.

The GPU tests read every stage's output back from the encode's workspace (`region`) and hand it to the `check_*` functions below; the
CPU test hands them the output of `emulate`, clean and with one synthesised fault at a time.  One set of checkers serves both, so a
fault the CPU test shows to be rejected is a fault the GPU tests would reject.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  Every bound is first order in u with its constants rounded up; the factor
(1 + 2^-10) at the end of each covers the products of first-order terms.  Nothing here was fitted to a kernel's output.

  sum of m numbers in ANY order (sequential, pairwise, the 64-lane butterfly): |err| <= (m - 1) u sum|a_i| (Higham, Accuracy and
  Stability of Numerical Algorithms, 4.2); the LayerNorm kernels add at most d = W / 64 + 8 numbers along any path from an element to the
  total (W / 64 per lane in the scalar path resp. 2 + W / 256 in the vectorised one, 6 butterfly levels, 3 more across k_head's four
  waves), so d u sum|a_i| bounds them -- far below the order-free (W - 1) u.

  rsqrtf: ROCm's HIP math documentation ("HIP math API", single-precision table) lists rsqrtf with a maximum error of 1 ULP.  The
  document is not part of the ROCm installation these tests were written against, so the figure could not be re-read there; RSQRT_ULP = 2
  is assumed instead, the limit of OpenCL's full profile for rsqrt, which the device library behind rsqrtf is built to meet.  One ULP is
  at most 2 u relative.

  dot product of K terms in any order with fp32 accumulation (MFMA steps, fma chains): (K + 2) u sum|a_k b_k| -- the order-free form of
  gemm_ln_ref.consumer_formula's (K / 32 + 2) u sum|x_k w_k|, which assumes the 32-deep MFMA steps of the 256 x 256 kernels; the patch
  embedding also runs on k_gemm_f16 and on the two fp32 kernels, whose step depths differ.
"""
import numpy as np

U32 = 2.0 ** -24
EPS = 1e-5
RSQRT_ULP = 2
SLACK = 1.0 + 2.0 ** -10
POISON = 0xA5
NP = {'f32': np.float32, 'f16': np.float16}


def ulp16(v):
    """Spacing of fp16 numbers at |v|, subnormals included: 2^(e - 10) for |v| in [2^e, 2^(e+1)), at least 2^-24."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    e = np.where(a == 0, -14, e - 1)
    return np.ldexp(1.0, np.maximum(e, -14) - 10)


def f16r(v):
    """float64 value of v rounded once to fp16 through fp32, as the kernels convert."""
    return np.asarray(v).astype(np.float32).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ workspace layout
def pad256(m):
    return (m + 255) // 256 * 256


def region(cfg, dtype, n, fold_on):
    """Byte offset and size of every region of vg_vit_encode's workspace, in the header's order x, h, qkv, mlp, patches, pe, x16, lnst --
    the closed form test_vit._workspace_bytes_closed_form pins, term by term.  `fold_on`: the handle runs the folded LayerNorm
    (fp16 tower, width % 256 == 0, VG_VIT_LN_FOLD not 0, not the fp16 stream).
    -> dict: name -> (offset, bytes); 'total'; the row counts M, Mp, P, Pp, K, Kp, T and qkv_ld (row stride of qkv in elements)."""
    W, es = cfg['width'], 2 if dtype == 'f16' else 4
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    K = 3 * cfg['patch'] ** 2
    Mp, Pp, Kp = pad256(n * T), pad256(n * (T - 1)), (K + 63) // 64 * 64
    fold = fold_on and dtype == 'f16' and W % 256 == 0
    sizes = [('x', Mp * W * 4), ('h', Mp * W * es), ('qkv', Mp * (3 * W + 256) * es), ('mlp', Mp * 4 * W * es),
             ('patches', Pp * Kp * es), ('pe', Pp * W * 4), ('x16', Mp * W * 2 if fold else 0), ('lnst', Mp * (W // 64) * 8 if fold else 0)]
    out, at = {}, 0
    for name, b in sizes:
        out[name] = (at, b)
        at += b
    out.update(total=at + 1024, M=n * T, Mp=Mp, P=n * (T - 1), Pp=Pp, K=K, Kp=Kp, T=T, qkv_ld=3 * W + 64 if dtype == 'f16' else 3 * W)
    return out


def pair_stream_from(cfg):
    """Smallest crop count at which vit_plan runs the fp16-pair stream on a folded tower of >= 2 layers: the compact class-row buffers
    (Mc = n padded to 256 rows: fp32 rows, two fp16 row sets, the hidden activations, W / 64 partials of 8 bytes per row) fit in the
    qkv region, and the query buffers (two fp16 row sets + partials) in the mlp region."""
    W = cfg['width']
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    for n in range(1, 4096):
        Mp, Mc = pad256(n * T), pad256(n)
        stats = (W // 64) * 8
        tail = Mc * (W * 4 + W * 2 + W * 2 + 4 * W * 2 + stats)
        query = Mc * (W * 2 + W * 2 + stats)
        if tail <= Mp * (3 * W + 256) * 2 and query <= Mp * 4 * W * 2:
            return n
    raise AssertionError('no crop count below 4096')


# ------------------------------------------------------------------------------------------------------------ float64 restatements
def im2col64(crops, ps, Kp):
    """P[(crop G G + py G + px)][c ps ps + i ps + j] = crops[crop, c, py ps + i, px ps + j]; columns 3 ps^2 .. Kp zero."""
    n, _, res, _ = crops.shape
    G = res // ps
    p = np.asarray(crops, dtype=np.float64).reshape(n, 3, G, ps, G, ps).transpose(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * ps * ps)
    return np.concatenate([p, np.zeros((p.shape[0], Kp - p.shape[1]))], 1)


def layernorm64(v, g, b):
    v = np.asarray(v, dtype=np.float64)
    mean = v.mean(1, keepdims=True)
    var = ((v - mean) ** 2).mean(1, keepdims=True)
    return (v - mean) / np.sqrt(var + EPS) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def embed_in64(pe, cls, pos, n, T):
    """Rows the embedding hands to ln_pre: (t == 0 ? class_embedding : pe[crop (T - 1) + t - 1]) + pos[t]  -> [n T, W]"""
    W = pos.shape[1]
    v = np.empty((n, T, W))
    v[:, 0] = np.asarray(cls, np.float64)
    v[:, 1:] = np.asarray(pe, np.float64)[:n * (T - 1)].reshape(n, T - 1, W)
    return (v + np.asarray(pos, np.float64)[None]).reshape(n * T, W)


def head64(xcls, g, b, proj):
    return layernorm64(xcls, g, b) @ np.asarray(proj, np.float64)


def fold_w1_exact(conv1, std3):
    """(256 / 255) sum_c conv1[n, c, p] / std_c in float64 from the float32 constants the handle holds -> [W, ps^2]"""
    W = conv1.shape[0]
    c = np.asarray(conv1, np.float64).reshape(W, 3, -1)
    s = np.asarray(std3, np.float32).astype(np.float64)
    return (256.0 / 255.0) * (c / s[None, :, None]).sum(1)


def fold64(conv1, pos, mean3, std3):
    """The single-channel fold as the comment above k_conv1_fold states it, from the float32 constants the handle holds:
    W1[n, p] = f16((256 / 255) sum_c conv1[n, c, p] / std_c),  b1[n] = - sum_c (mean_c / std_c) sum_p conv1[n, c, p],
    pos1[t] = pos[t] + (t > 0 ? b1 : 0).  -> (W1 [W, ps^2] as float64, pos1 [T, W] float64, b1 [W])
    W1 is the float64 value rounded ONCE to fp16.  The kernel's source converts double -> float -> fp16; read back through one-hot
    patch rows (test_single_channel_weight_read_back) the compiled kernel holds the once-rounded value in every element, also in the few
    per 100 000 where the two-step conversion lands one fp16 ulp away (a double rounding: the float lies exactly on an fp16 tie).  Either
    is a correct kernel, so the checkers take the once-rounded value and allow the difference to the two-step one (fold_w1_slack)."""
    W = conv1.shape[0]
    c = np.asarray(conv1, np.float64).reshape(W, 3, -1)
    m, s = np.asarray(mean3, np.float32).astype(np.float64), np.asarray(std3, np.float32).astype(np.float64)
    W1 = fold_w1_exact(conv1, std3).astype(np.float16).astype(np.float64)
    b1 = -((c * (m / s)[None, :, None]).sum((1, 2)))
    pos1 = np.asarray(pos, np.float64).copy()
    pos1[1:] += b1[None]
    return W1, pos1, b1


def fold_w1_slack(conv1, std3):
    """|f16(x) - f16(f32(x))| per element of W1's float64 value x: zero except where the two-step conversion double-rounds."""
    x = fold_w1_exact(conv1, std3)
    return np.abs(x.astype(np.float16).astype(np.float64) - f16r(x))


# ------------------------------------------------------------------------------------------------------------ bounds
def bound_dot(A, B):
    """|fp32-accumulated A B^T - exact| per element, A [M, K], B [N, K] exact operands: (K + 2) u sum_k |a_k b_k| (module docstring)."""
    K = A.shape[1]
    return (K + 2) * U32 * (np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)).T) * SLACK


def bound_ln(v, g, b, out='f32', dv=None, parts=False):
    """Per-element bound of |kernel LayerNorm(v) - layernorm64(v)| for rows v [R, W] the kernel reads exactly, in the kernels' arithmetic
    (k_layernorm, both LayerNorms of k_embed_lnpre, k_head's ln_post):

      mean:   tree sum of W numbers, depth d = W / 64 + 8, and one division: dm = (d + 2) u mean|v|
      dev_i = v_i - mean: one rounding, u |dev_i|, plus dm
      var:    squares (2 u relative each, from dev_i's rounding and the product's), tree sum (d u), division and + eps (2 u): (d + 8) u
              relative at most; the wrong centre adds dm^2 (sum of (v_i - m')^2 = sum of (v_i - m)^2 + W (m - m')^2)
      rstd:   half the relative error of var + eps, plus RSQRT_ULP ulps of 2 u each
      y_i = dev_i rstd g_i + b_i: three roundings (fewer where the compiler contracts to fma): 2 u |dev_i rstd g_i| + u |y_i|
    The last of these, u |y_i|, is the fp32 output's own rounding; then the narrower output's: none ('f32'), one fp16 rounding ('f16': half an fp16 ulp at the computed value), or the pair
    ('pair': hi + lo = y up to the rounding of lo = f16(y - hi), |lo| <= 2^-11 |y|: 2^-22 |y|, at least half the fp16 subnormal spacing,
    2^-25).
    dv (optional, [R, W]): a bound of what the kernel's input rows may differ from v by (an earlier stage's error), propagated to first
    order: dev_i moves by dv_i + mean(dv), var by (2 / W) sum |dev_i| (dv_i + mean dv) + mean((dv + mean dv)^2).
    parts: -> (bound, the output rounding's share of it) instead of the bound alone."""
    v = np.asarray(v, np.float64)
    gs, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    g = np.abs(gs)
    W = v.shape[1]
    d = W // 64 + 8
    mean = v.mean(1, keepdims=True)
    dev = v - mean
    var = (dev ** 2).mean(1, keepdims=True)
    r = 1.0 / np.sqrt(var + EPS)
    y = dev * r * gs + b
    dm = (d + 2) * U32 * np.abs(v).mean(1, keepdims=True)
    rho = 0.5 * ((d + 8) * U32 + dm ** 2 / (var + EPS)) + RSQRT_ULP * 2 * U32
    lin = np.abs(dev) * r * g
    e = g * r * (dm + U32 * np.abs(dev)) + lin * (rho + 2 * U32)
    if dv is not None:
        dd = np.asarray(dv, np.float64)
        dd = dd + dd.mean(1, keepdims=True)
        rel = 0.5 * ((2.0 / W) * (np.abs(dev) * dd).sum(1, keepdims=True) + (dd ** 2).mean(1, keepdims=True)) / (var + EPS)
        e = e + g * r * (dd * (1 + rel) + np.abs(dev) * rel)
    e = e * SLACK
    rnd = U32 * (np.abs(y) + e)                      # the last addition's rounding: the fp32 output's own
    if out == 'f16':
        rnd = rnd + ulp16(np.abs(y) + e + rnd) / 2
    elif out == 'pair':
        rnd = rnd + np.maximum(2.0 ** -22 * (np.abs(y) + e + rnd), 2.0 ** -25)
    else:
        assert out == 'f32', out
    return (e + rnd, rnd) if parts else e + rnd


def bound_head(xcls, g, b, proj, dv=None):
    """k_head: ln_post in fp32 (bound_ln; the normalised row stays fp32 in LDS), then an fma chain over W per output: the LayerNorm's error
    times |proj|, plus the dot product's own (W + 2) u sum |ln_i proj_ij|."""
    p = np.abs(np.asarray(proj, np.float64))
    ln = layernorm64(xcls, g, b)
    return bound_ln(xcls, g, b, 'f32', dv) @ p + (xcls.shape[1] + 2) * U32 * (np.abs(ln) @ p) * SLACK


def worst(got, want, bound, what, rounding=None):
    """AssertionError where an element is not finite or |got - want| exceeds its bound (a zero bound demands equality).
    -> the worst error / bound ratio.  `rounding`: the share of the bound that is the output's own rounding (fp16, pair).  A correct kernel
    attains that share (a correctly rounded value sits up to half an ulp from the exact one), so the ratio that tells how much of the
    DERIVED arithmetic bound was used leaves it out on both sides: max(|err| - rounding, 0) / (bound - rounding)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite values'
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        at = np.argwhere(bad)[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements out of bound; worst |err| / bound = '
                             f'{(err / np.maximum(bound, 1e-300)).max():.3g}, first at {at}')
    if rounding is not None:
        err, bound = np.maximum(err - rounding, 0), bound - rounding
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------------------ the checkers
# A `case` is a dict: cfg (width, patch, resolution, output_dim), n, dtype ('f32' / 'f16': the tower's compute type), stream ('f32' /
# 'f16' / 'pair': the form k_embed_lnpre writes), kind (0 / 1: CHW crops; 3: single-channel patch rows), crops (the input array),
# w (name -> float32 array, state_dict names), norm ((mean3, std3), kind 3 only).  `got` is a dict of the stages' outputs:
# patches, pe, x (or hi and lo), h1, h2, feat -- whatever the test could observe.

def stream_value(case, got):
    """The residual stream k_embed_lnpre wrote, as float64 [Mp, W]."""
    if case['stream'] == 'pair':
        return got['hi'].astype(np.float64) + got['lo'].astype(np.float64)
    return got['x'].astype(np.float64)


def gemm_operands(case, got):
    """Exact operands of the patch-embedding GEMM -> (A [P, K'] from the patch rows the GPU wrote or was given, B [W, K'], pos table)."""
    cfg, w = case['cfg'], case['w']
    W, P = cfg['width'], case['n'] * ((cfg['resolution'] // cfg['patch']) ** 2)
    if case['kind'] == 3:
        W1, pos1, _ = fold64(w['conv1.weight'], w['positional_embedding'], *case['norm'])
        return np.asarray(case['crops'], np.float64)[:P], W1, pos1
    A = got['patches'].astype(np.float64)[:P]
    B = np.asarray(w['conv1.weight']).reshape(W, -1).astype(NP[case['dtype']]).astype(np.float64)
    B = np.concatenate([B, np.zeros((W, A.shape[1] - B.shape[1]))], 1)
    return A, B, np.asarray(w['positional_embedding'], np.float64)


def check_patches(case, got):
    """The patches region equals the float64 im2col after the one rounding to the compute type bit for bit, K-padding columns included."""
    cfg = case['cfg']
    K = 3 * cfg['patch'] ** 2
    Kp = (K + 63) // 64 * 64
    want = im2col64(case['crops'], cfg['patch'], Kp).astype(np.float32).astype(NP[case['dtype']])
    P = want.shape[0]
    have = got['patches'][:P]
    assert have.dtype == want.dtype and have.shape == want.shape, (have.dtype, have.shape, want.shape)
    assert (have[:, K:].view(np.uint16 if case['dtype'] == 'f16' else np.uint32) == 0).all(), 'K-padding columns of the patch rows are not zero'
    same = have.view(np.uint16 if case['dtype'] == 'f16' else np.uint32) == want.view(np.uint16 if case['dtype'] == 'f16' else np.uint32)
    same |= (have == 0) & (want == 0)                     # (-0.0 from a crop that holds -0.0)
    assert same.all(), f'patch rows: {int((~same).sum())} elements differ from im2col, first at {np.argwhere(~same)[0].tolist()}'
    return 0.0


def check_pe(case, got):
    A, B, _ = gemm_operands(case, got)
    bound = bound_dot(A, B)
    if case['kind'] == 3:
        bound = bound + np.abs(A) @ fold_w1_slack(case['w']['conv1.weight'], case['norm'][1]).T
    return worst(got['pe'][:A.shape[0]], A @ B.T, bound, 'patch embedding')


def check_stream(case, got):
    """Rows < M of the stream against the float64 embedding + ln_pre of the GPU's OWN patch-embedding rows; rows M .. Mp exactly zero;
    the pair's lo within half an ulp of its hi."""
    cfg, w, n = case['cfg'], case['w'], case['n']
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    M = n * T
    _, _, pos = gemm_operands(case, got)
    if case['kind'] != 3:
        # the kernel adds src + pos in fp32: ONE rounding, which float32 arithmetic restates exactly -- the LayerNorm reads these rows
        vin = embed_in64(got['pe'], w['class_embedding'], pos, n, T).astype(np.float32).astype(np.float64)
        dv = None
    else:
        # kind 3: the table pos + b1 was rounded to fp32 by k_conv1_fold (b1's own rounding, then the sum's), and the test cannot read it
        # back: u |b1| + u |pos + b1|, and u |v| for the kernel's addition, enter as the input's uncertainty
        vin = embed_in64(got['pe'], w['class_embedding'], pos, n, T)
        b1 = pos - np.asarray(w['positional_embedding'], np.float64)
        dv = np.tile(U32 * (np.abs(pos) + np.abs(b1)), (n, 1)) + U32 * np.abs(vin)
    want = layernorm64(vin, w['ln_pre.weight'], w['ln_pre.bias'])
    bound, rnd = bound_ln(vin, w['ln_pre.weight'], w['ln_pre.bias'], case['stream'], dv, parts=True)
    xs = stream_value(case, got)
    ratio = worst(xs[:M], want, bound, f"stream after ln_pre ({case['stream']})", rnd)
    for name in (('hi', 'lo') if case['stream'] == 'pair' else ('x',)):
        pad = got[name][M:]
        assert pad.size == 0 or (pad.view(np.uint16 if pad.dtype == np.float16 else np.uint32) == 0).all(), \
            f'padding rows of the stream ({name}) are not zero'
    if case['stream'] == 'pair':
        assert (np.abs(got['lo'].astype(np.float64)) <= ulp16(got['hi']) / 2).all(), 'lo beyond half an ulp of hi'
    return ratio


def check_ln(rows, h, g, b, out, what):
    """h (the kernel's output for `rows`, which it read exactly) against float64 LayerNorm."""
    rows = np.asarray(rows, np.float64)
    bound, rnd = bound_ln(rows, g, b, out, parts=True)
    return worst(h[:rows.shape[0]], layernorm64(rows, g, b), bound, what, rnd)


def check_feat(case, got, cls_rows=None):
    """Features against the float64 head of the GPU's own class-token rows."""
    cfg, w, n = case['cfg'], case['w'], case['n']
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    xc = stream_value(case, got)[:n * T:T] if cls_rows is None else np.asarray(cls_rows, np.float64)
    args = (xc, w['ln_post.weight'], w['ln_post.bias'], w['proj'])
    return worst(got['feat'], head64(*args), bound_head(*args), 'features from the GPU rows')


def check_chain(case, got):
    """Features of a zero-layer tower against the all-float64 chain from the rounded operands, within the summed bound: the GEMM's bound
    enters ln_pre as dv, ln_pre's bound enters the head as dv."""
    cfg, w, n = case['cfg'], case['w'], case['n']
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    if case['kind'] == 3:
        A, B, pos = gemm_operands(case, got)
    else:
        K = 3 * cfg['patch'] ** 2
        A = im2col64(case['crops'], cfg['patch'], (K + 63) // 64 * 64).astype(np.float32).astype(NP[case['dtype']]).astype(np.float64)
        _, B, pos = gemm_operands(case, dict(got, patches=A))
    pe = A @ B.T
    v = embed_in64(pe, w['class_embedding'], pos, n, T)
    dv = U32 * np.abs(v) + 2 * U32 * np.abs(np.tile(pos, (n, 1)))
    dv.reshape(n, T, -1)[:, 1:] += bound_dot(A, B).reshape(n, T - 1, -1)
    x = layernorm64(v, w['ln_pre.weight'], w['ln_pre.bias'])
    ex = bound_ln(v, w['ln_pre.weight'], w['ln_pre.bias'], case['stream'], dv)
    args = (x[::T], w['ln_post.weight'], w['ln_post.bias'], w['proj'])
    return worst(got['feat'], head64(*args), bound_head(*args, dv=ex[::T]), 'features from the float64 chain')


def check_zero_layer(case, got):
    """Every assertion on a zero-layer encode -> dict of worst error / bound ratios."""
    r = {}
    if case['kind'] != 3:
        check_patches(case, got)
    r['pe'] = check_pe(case, got)
    r['x'] = check_stream(case, got)
    r['feat'] = check_feat(case, got)
    r['chain'] = check_chain(case, got)
    return r


def check_probe(case, got):
    """The one-layer probe tower (identity in_proj, zero out_proj / c_proj): the stream survives the block, qkv[:, :W] is ln_1 of it and,
    where a separate LayerNorm launch ran, h is ln_2 of it."""
    w = case['w']
    p = 'transformer.resblocks.0.'
    cfg, n = case['cfg'], case['n']
    M = n * ((cfg['resolution'] // cfg['patch']) ** 2 + 1)
    r = {'pe': check_pe(case, got), 'x': check_stream(case, got)}
    rows = stream_value(case, got)[:M]
    out = 'f32' if case['dtype'] == 'f32' else 'f16'
    r['ln_1'] = check_ln(rows, got['h1'], w[p + 'ln_1.weight'], w[p + 'ln_1.bias'], out, 'ln_1 (qkv[:, :W])')
    if 'h2' in got:
        r['ln_2'] = check_ln(rows, got['h2'], w[p + 'ln_2.weight'], w[p + 'ln_2.bias'], out, 'ln_2 (h)')
    return r


# ------------------------------------------------------------------------------------------------------------ inputs
FAMILIES = ('gauss', 'offset', 'massive', 'const')
SIGMAS = (1.0, 0.01, 2.0, 0.1, 0.5)            # a row of every scale in any five consecutive tokens: var + eps is not var for 0.01


def family_rows(family, T, W, rng):
    """T distinct rows [T, W] float64 the embedding hands to ln_pre when the patch embedding is zero: 'gauss'; 'offset' (row mean = 50 x row
    std, alternating sign); 'massive' (three channels 100 x the rest); 'const' (as gauss, row 2 constant: variance 0, output = shift)."""
    s = np.array([SIGMAS[t % len(SIGMAS)] for t in range(T)])[:, None]
    R = s * rng.standard_normal((T, W)) + s * rng.uniform(-1, 1, (T, 1))
    if family == 'offset':
        R += 50 * s * np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None]
    elif family == 'massive':
        R[:, [7, W // 2 + 3, W - 5]] = 100 * s * np.array([1.0, -1.0, 1.0]) * rng.uniform(0.8, 1.2, (T, 3))
    elif family == 'const':
        R[2] = 3.0
    else:
        assert family == 'gauss', family
    return R


def make_weights(cfg, family, seed, layers=0, probe=True, stream_scale=1.0):
    """Hand-built tower weights (float32 arrays by state_dict name): LayerNorm gains 0.3 .. 2.5 and shifts +- 0.8, all different; class
    embedding of order 1; positional table = the family's rows (row 0 less the class embedding), so crops of zeros put exactly those
    rows into ln_pre.  layers >= 1, probe: in_proj = three stacked identities with zero bias, out_proj and c_proj zero, c_fc random.
    layers >= 1, not probe: out_proj and c_proj zero, everything else random.
    stream_scale < 1: ln_pre's gain and its shift's spread are multiplied by it (shift centred at 0.5), so the rows of the stream that ln_1,
    ln_2 and ln_post read have a variance comparable with the LayerNorm epsilon -- the only inputs on which those kernels' eps shows."""
    rng = np.random.default_rng(seed)
    W, ps, D = cfg['width'], cfg['patch'], cfg['output_dim']
    T = (cfg['resolution'] // ps) ** 2 + 1
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    gain = lambda: f(rng.uniform(0.3, 2.5, W))
    shift = lambda: f(rng.uniform(-0.8, 0.8, W))
    cls = f(0.5 * rng.standard_normal(W))
    pos = family_rows(family, T, W, rng)
    pos[0] -= cls
    w = {'conv1.weight': f(rng.standard_normal((W, 3, ps, ps)) * (3 * ps * ps) ** -0.5), 'class_embedding': cls,
         'positional_embedding': f(pos), 'ln_pre.weight': gain() * np.float32(stream_scale),
         'ln_pre.bias': f(shift() * stream_scale + (0.5 if stream_scale != 1.0 else 0.0)), 'ln_post.weight': gain(),
         'ln_post.bias': shift(), 'proj': f(rng.standard_normal((W, D)) * W ** -0.5)}
    for l in range(layers):
        p = f'transformer.resblocks.{l}.'
        w[p + 'ln_1.weight'], w[p + 'ln_1.bias'], w[p + 'ln_2.weight'], w[p + 'ln_2.bias'] = gain(), shift(), gain(), shift()
        if probe:
            w[p + 'attn.in_proj_weight'] = f(np.concatenate([np.eye(W)] * 3))
            w[p + 'attn.in_proj_bias'] = f(np.zeros(3 * W))
        else:
            w[p + 'attn.in_proj_weight'] = f(rng.standard_normal((3 * W, W)) * W ** -0.5)
            w[p + 'attn.in_proj_bias'] = f(rng.uniform(-0.1, 0.1, 3 * W))
        w[p + 'attn.out_proj.weight'], w[p + 'attn.out_proj.bias'] = f(np.zeros((W, W))), f(np.zeros(W))
        w[p + 'mlp.c_fc.weight'] = f(rng.standard_normal((4 * W, W)) * (2 * W) ** -0.5)
        w[p + 'mlp.c_fc.bias'] = f(rng.uniform(-0.1, 0.1, 4 * W))
        w[p + 'mlp.c_proj.weight'], w[p + 'mlp.c_proj.bias'] = f(np.zeros((W, 4 * W))), f(np.zeros(W))
    return w


CROP_SCALES = (0.0, 1.0, 0.05, 3.0)


def make_crops(cfg, n, seed, dtype=np.float32):
    """CHW crops [n, 3, res, res]: crop 0 all zeros (its tokens are the positional rows themselves), the others gaussian at three scales."""
    rng = np.random.default_rng(seed)
    res = cfg['resolution']
    s = np.array([CROP_SCALES[c % len(CROP_SCALES)] for c in range(n)])[:, None, None, None]
    return np.ascontiguousarray((s * rng.standard_normal((n, 3, res, res))).astype(np.float32).astype(dtype))


def make_levels(cfg, n, seed):
    """Single-channel patch rows [P padded to 256, patch^2] fp16 holding u / 256, u uniform in 0 .. 255; patch 0 all 0, patch 1 all 255."""
    rng = np.random.default_rng(seed)
    pp = cfg['patch'] ** 2
    P = n * (cfg['resolution'] // cfg['patch']) ** 2
    u = rng.integers(0, 256, (pad256(P), pp))
    u[0], u[1] = 0, 255
    u[P:] = 0
    return u, (u / 256.0).astype(np.float16)


def levels_as_crops64(cfg, n, u, norm):
    """The CHW crops [n, 3, res, res] (float64) whose three channels hold (u / 255 - mean_c) / std_c of the single-channel rows u."""
    ps, G = cfg['patch'], cfg['resolution'] // cfg['patch']
    img = u[:n * G * G].reshape(n, G, G, ps, ps).transpose(0, 1, 3, 2, 4).reshape(n, 1, G * ps, G * ps) / 255.0
    m, s = np.asarray(norm[0], np.float32).astype(np.float64), np.asarray(norm[1], np.float32).astype(np.float64)
    return (img - m[None, :, None, None]) / s[None, :, None, None]


def levels_as_crops(cfg, n, u, norm):
    return np.ascontiguousarray(levels_as_crops64(cfg, n, u, norm).astype(np.float32))


def fold_equivalence(case3, case0, u):
    """The single-channel path (kind 3) and the three-channel path (kind 0, fp16 tower) of one zero-layer tower against the embedding both
    stand for: v = conv1(x) + pos with x_c = (u / 255 - mean_c) / std_c in real arithmetic, then ln_pre.
    -> (want [M, W] float64, bound of the kind-3 stream, bound of the kind-0 stream), the bounds = bound_ln with the input uncertainty
      kind 3: the GEMM's bound + (u / 256) (|W1 - f16(W1)| + fold_w1_slack) (the fold's rounding, measured on the float64 formula) + the fp32 roundings of
              b1 and pos + b1 + the kernel's addition
      kind 0: the GEMM's bound + |x - f16(x)| |f16(conv1)| + |x| |conv1 - f16(conv1)| (the operands' roundings, measured) + the addition.
    The two streams then differ by at most the sum of the two."""
    cfg, w, n = case3['cfg'], case3['w'], case3['n']
    W, ps = cfg['width'], cfg['patch']
    T = (cfg['resolution'] // ps) ** 2 + 1
    P = n * (T - 1)
    g, b = w['ln_pre.weight'], w['ln_pre.bias']
    c = np.asarray(w['conv1.weight'], np.float64).reshape(W, 3, -1)
    W1x = fold_w1_exact(w['conv1.weight'], case3['norm'][1])
    W1r, pos1, b1 = fold64(w['conv1.weight'], w['positional_embedding'], *case3['norm'])
    A3 = np.asarray(case3['crops'], np.float64)[:P]
    v = embed_in64(A3 @ W1x.T, w['class_embedding'], pos1, n, T)
    rnd = U32 * np.abs(v) + np.tile(U32 * (np.abs(pos1) + np.abs(b1)), (n, 1))
    d3 = rnd.copy()
    d3.reshape(n, T, W)[:, 1:] += (bound_dot(A3, W1r) + A3 @ (np.abs(W1x - W1r) + fold_w1_slack(w['conv1.weight'], case3['norm'][1])).T).reshape(n, T - 1, W)
    x64 = im2col64(levels_as_crops64(cfg, n, u, case3['norm']), ps, 3 * ps * ps)
    A0 = im2col64(case0['crops'], ps, 3 * ps * ps).astype(np.float32).astype(np.float16).astype(np.float64)
    B = c.reshape(W, -1)
    B0 = f16r(B)
    d0 = U32 * np.abs(v) + np.zeros_like(v)
    d0.reshape(n, T, W)[:, 1:] += (bound_dot(A0, B0) + np.abs(A0 - x64) @ np.abs(B0).T + np.abs(x64) @ np.abs(B - B0).T).reshape(n, T - 1, W)
    return layernorm64(v, g, b), bound_ln(v, g, b, 'f32', d3), bound_ln(v, g, b, 'f32', d0)


# ------------------------------------------------------------------------------------------------------------ float32 emulations
FAULTS_IM2COL = ('kpad_stale', 'im2col_ij', 'im2col_cstride')
FAULTS_EMBED = ('pos_t+1', 'pos_t-1', 'cls_for_t1', 'patch_for_t0', 'crop+1', 'crop-1', 'pad_stale')
FAULTS_LN = ('gain_by_lane', 'gain_shift_swapped', 'no_eps', 'var_wm1', 'mean_256')
FAULTS_FOLD = ('b1_on_cls', 'no_256_255', 'norm_shift_channel')
FAULTS_FUSED = ('round_before_ln1',)
F32 = np.float32


def _wave_sum(p):
    """vg_wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 on [rows, 64] float32 -> [rows]"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ o]
    return p[:, 0]


def _lane_sum(v, fn, vec):
    """Per-lane partial sums of fn(v) in the kernel's order -> [rows, 64]: scalar path column lane + 64 i, i ascending; vectorised path
    columns (i 64 + lane) 4 .. + 3 as (a + b) + (c + d), i ascending."""
    rows, W = v.shape
    t = fn(v)
    s = np.zeros((rows, 64), F32)
    if vec:
        t = t.reshape(rows, W // 256, 64, 4)
        for i in range(W // 256):
            s = s + ((t[:, i, :, 0] + t[:, i, :, 1]) + (t[:, i, :, 2] + t[:, i, :, 3]))
    else:
        t = t.reshape(rows, W // 64, 64)
        for i in range(W // 64):
            s = s + t[:, i, :]
    return s


def emu_ln(v, g, b, fault=None, block=False):
    """One LayerNorm in float32 in the kernels' summation order (block: k_head's 256-thread form) -> float32 [rows, W] before any
    output rounding."""
    v, g, b = np.asarray(v, F32), np.asarray(g, F32), np.asarray(b, F32)
    rows, W = v.shape
    vec = W % 256 == 0 and W <= 1024 and not block
    lane = (np.arange(W) // 4) % 64 if vec else np.arange(W) % 64
    if fault == 'gain_by_lane':
        g, b = g[lane], b[lane]
    if fault == 'gain_shift_swapped':
        g, b = b, g
    ncol = min(W, 256) if fault == 'mean_256' else W

    def total(t):
        if block:                                        # thread tid sums columns tid + 256 k; four waves; ((r0 + r1) + r2) + r3
            pad = np.zeros((rows, (W + 255) // 256 * 256), F32)
            pad[:, :W] = t
            per = pad.reshape(rows, -1, 256)
            s = np.zeros((rows, 256), F32)
            for k in range(per.shape[1]):
                s = s + per[:, k]
            red = [_wave_sum(s[:, 64 * k:64 * k + 64]) for k in range(4)]
            return ((red[0] + red[1]) + red[2]) + red[3]
        return _wave_sum(_lane_sum(t, lambda a: a, vec))
    keep = (np.arange(W) < ncol).astype(F32)
    mean = total(v * keep) / F32(ncol)
    dev = v - mean[:, None]
    var = total(dev * dev) / F32(W - 1 if fault == 'var_wm1' else W)
    with np.errstate(divide='ignore', invalid='ignore'):
        rstd = F32(1) / np.sqrt(var + (F32(0) if fault == 'no_eps' else F32(1e-5)))
        return (dev * rstd[:, None] * g + b).astype(F32)


def emu_im2col(crops, ps, Kp, dtype, fault=None):
    """k_im2col's index arithmetic per output element; the buffer holds the poison byte where the kernel does not write."""
    n, _, res, _ = crops.shape
    G, K = res // ps, 3 * ps * ps
    idx = np.arange(n * G * G * Kp)
    col, row = idx % Kp, idx // Kp
    px, py, crop = row % G, (row // G) % G, row // (G * G)
    j, i, c = col % ps, (col // ps) % ps, np.minimum(col // (ps * ps), 2)
    if fault == 'im2col_ij':
        i, j = j, i
    nch = 1 if fault == 'im2col_cstride' else 3          # ((crop * 3 + c) * res + y) * res + x with 1 for the 3
    src = ((crop * nch + c) * res + (py * ps + i)) * res + px * ps + j
    out = np.asarray(crops).reshape(-1)[np.minimum(src, crops.size - 1)].astype(np.float32).astype(NP[dtype])
    stale = np.frombuffer(bytes([POISON]) * out.itemsize, dtype=NP[dtype])[0]
    out[col >= K] = stale if fault == 'kpad_stale' else 0
    return out.reshape(n * G * G, Kp)


def emu_dot(A, B):
    """fp32-accumulated A B^T in 16-deep steps (the narrowest MFMA of the kernels): float32 [M, N]"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    acc = np.zeros((A.shape[0], B.shape[0]), F32)
    for k in range(0, A.shape[1], 16):
        acc = (acc + (A[:, k:k + 16] @ B[:, k:k + 16].T).astype(F32)).astype(F32)
    return acc


def emu_fold(conv1, pos, mean3, std3, fault=None):
    """k_conv1_fold with float64 accumulation -> (W1 fp16 [W, ps^2], pos1 float32 [T, W])"""
    W = conv1.shape[0]
    c = np.asarray(conv1, np.float64).reshape(W, 3, -1)
    m, s = np.asarray(mean3, F32).astype(np.float64), np.asarray(std3, F32).astype(np.float64)
    if fault == 'norm_shift_channel':
        m, s = np.roll(m, 1), np.roll(s, 1)               # channel (c + 1) % 3 meets channel c's constants
    k = 1.0 if fault == 'no_256_255' else 256.0 / 255.0
    W1 = (k * (c[:, 0] / s[0] + c[:, 1] / s[1] + c[:, 2] / s[2])).astype(F32).astype(np.float16)
    b1 = (-(c[:, 0] * (m[0] / s[0]) + c[:, 1] * (m[1] / s[1]) + c[:, 2] * (m[2] / s[2])).sum(1)).astype(F32)
    pos1 = np.asarray(pos, F32).copy()
    pos1[0 if fault == 'b1_on_cls' else 1:] += b1[None]
    return W1, pos1


def emulate(case, fault=None, layers=0):
    """The stages of a zero-layer (or one-layer probe) encode in float32, kernel by kernel, optionally with ONE synthesised fault
    -> `got` as the GPU tests read it back."""
    cfg, w, n, dt = case['cfg'], case['w'], case['n'], case['dtype']
    W, ps = cfg['width'], cfg['patch']
    T = (cfg['resolution'] // ps) ** 2 + 1
    M, P, Mp = n * T, n * (T - 1), pad256(n * T)
    got = {}
    pos = np.asarray(w['positional_embedding'], F32)
    if case['kind'] == 3:
        A = np.asarray(case['crops'])[:P]
        B, pos = emu_fold(w['conv1.weight'], pos, *case['norm'], fault=fault if fault in FAULTS_FOLD else None)
    else:
        K = 3 * ps * ps
        Kp = (K + 63) // 64 * 64
        A = got['patches'] = emu_im2col(case['crops'], ps, Kp, dt, fault if fault in FAULTS_IM2COL else None)
        B = np.zeros((W, Kp), NP[dt])
        B[:, :K] = np.asarray(w['conv1.weight']).reshape(W, K).astype(NP[dt])
    with np.errstate(invalid='ignore', over='ignore'):
        pe = got['pe'] = emu_dot(A, B)
    # k_embed_lnpre
    crop, t = np.arange(M) // T, np.arange(M) % T
    tp = (t + (1 if fault == 'pos_t+1' else -1 if fault == 'pos_t-1' else 0)) % T
    cs = (crop + (1 if fault == 'crop+1' else -1 if fault == 'crop-1' else 0)) % n
    is_cls = (t == 0) if fault not in ('cls_for_t1', 'patch_for_t0') else (t <= 1) if fault == 'cls_for_t1' else np.zeros(M, bool)
    src = pe[np.clip(cs * (T - 1) + np.maximum(t - 1, 0), 0, P - 1)]
    src[is_cls] = np.asarray(w['class_embedding'], F32)
    v = (src + pos[tp]).astype(F32)
    lnf = fault if fault in FAULTS_LN else None
    o = emu_ln(v, w['ln_pre.weight'], w['ln_pre.bias'], lnf)
    stale = np.frombuffer(bytes([POISON]) * 4, dtype=F32)[0]
    fill = stale if fault == 'pad_stale' else F32(0)
    if case['stream'] == 'f16':
        got['x'] = np.zeros((Mp, W), np.float16)
        if fault == 'pad_stale':
            got['x'].view(np.uint8)[:] = POISON
        got['x'][:M] = o.astype(np.float16)
        nxt = got['x'][:M].astype(F32)
    elif case['stream'] == 'pair':
        hi = o.astype(np.float16)
        lo = (o - hi.astype(F32)).astype(np.float16)
        got['hi'], got['lo'] = np.full((Mp, W), fill, np.float16), np.full((Mp, W), fill, np.float16)
        got['hi'][:M], got['lo'][:M] = hi, lo
        nxt = hi.astype(F32) + lo.astype(F32)
    else:
        got['x'] = np.full((Mp, W), fill, F32)
        got['x'][:M] = o
        nxt = o
    if layers:
        p = 'transformer.resblocks.0.'
        hdt = NP[dt]
        fused_in = nxt.astype(np.float16).astype(F32) if fault == 'round_before_ln1' else nxt
        got['h1'] = emu_ln(fused_in, w[p + 'ln_1.weight'], w[p + 'ln_1.bias'], lnf).astype(hdt)
        got['h2'] = emu_ln(nxt, w[p + 'ln_2.weight'], w[p + 'ln_2.bias'], lnf).astype(hdt)
    # k_head on the class rows
    sm = emu_ln(nxt[::T], w['ln_post.weight'], w['ln_post.bias'], lnf, block=True).astype(np.float64)
    proj = np.asarray(w['proj'], F32).astype(np.float64)
    a = np.zeros((n, proj.shape[1]), F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(W):
            a = (sm[:, i:i + 1] * proj[i][None] + a.astype(np.float64)).astype(F32)
    got['feat'] = a
    return got
