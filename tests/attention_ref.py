"""Plain float64 reference, derived error bounds, input families and checker of the attention kernels (vg_attention_rows; csrc/vit.hip
k_attention_f16, k_attention_f16_long, k_attention_f32), shared by tests/test_attention.py, the two older attention tests and the CPU
test of the checker itself.

The operation is softmax(q k^T / 8) v per (crop, head), head dimension 64 (model.py:175-187 via nn.MultiheadAttention).  The reference
is computed from the same fp16 (or fp32) input bits the kernel reads, in float64 throughout.  `emulate` restates the ROUNDING of the
fp16 kernels on the CPU (fp32 logits, fp16 probabilities, fp32 accumulation, fp16 output; one pass or 64-key online blocks) and can
synthesise the outputs of wrong kernels, so that the checker is tested without running a broken kernel.

Layouts: qkv [n_crops * T, ld] with q | k | v at columns 0 | W | 2W, columns 3W .. ld padding; out [n_crops * T, W]."""
import numpy as np
import torch

U16 = 2.0 ** -11          # unit roundoff of fp16
U32 = 2.0 ** -24          # unit roundoff of fp32
GUARD = 7776.0            # sentinel of the guard rows around `out` (exact in fp16)
FAMILIES = ('gauss', 'hot', 'sink', 'sink_last', 'uniform', 'onehot')
FLAT_OLD = 2e-3           # the flat bound the attention tests used before: |err| < 2e-3 max|v|


def n_tiles(T):
    return (T + 31) // 32


# ------------------------------------------------------------------------------------------------------------------- inputs
def make_qkv(family, n_crops, T, W, H, ld, seed, dtype=torch.float16):
    """Seeded inputs [n_crops * T, ld]; padding columns 3W .. ld are NaN.  `family` is one name or a list of names, one per crop
    (consecutive items of a persistent launch then carry different data).  -> (qkv, perm) with perm [n_crops, H, T] the attended key
    of every row for 'onehot' crops (None without one).

      gauss      q 1.5, k 1.0, v 2.0 x N(0,1): logits of standard deviation 1.5
      hot        q 6.0, k 3.0 x N(0,1): |logit| up to ~100
      sink       q = 2 N + 24 u, k = N, k[0] += 20 u, u a unit vector per head: every row's maximum at key 0, ~60 above the rest
      sink_last  the same with the sink at key T - 1 (the last, partly masked key block)
      uniform    q = 0, v = 2 N + 3: every row is the mean of v[:T]
      onehot     k = 4 E, q = 4 E[perm], E random +-1: the attended key's logit is 128, the others N(0, 16): out row = v[perm[row]]"""
    fams = [family] * n_crops if isinstance(family, str) else list(family)
    assert len(fams) == n_crops and ld >= 3 * W and H * 64 == W
    g = torch.Generator().manual_seed(seed)
    qkv = torch.full((n_crops, T, ld), float('nan'), dtype=torch.float32)
    perms = None
    for c, fam in enumerate(fams):
        q, k, v = [torch.randn(T, H, 64, generator=g) for _ in range(3)]
        v = v * 2.0
        if fam == 'gauss':
            q = q * 1.5
        elif fam == 'hot':
            q, k = q * 6.0, k * 3.0
        elif fam in ('sink', 'sink_last'):
            u = torch.randn(H, 64, generator=g)
            u = u / u.norm(dim=-1, keepdim=True)
            q = q * 2.0 + 24.0 * u
            k[0 if fam == 'sink' else T - 1] += 20.0 * u
        elif fam == 'uniform':
            q = torch.zeros_like(q)
            v = v + 3.0
        elif fam == 'onehot':
            E = torch.randint(0, 2, (T, H, 64), generator=g).float() * 2 - 1
            perm = torch.stack([torch.randperm(T, generator=g) for _ in range(H)])        # [H, T]
            k = 4.0 * E
            q = 4.0 * torch.gather(E, 0, perm.t()[:, :, None].expand(T, H, 64))
            if perms is None:
                perms = torch.zeros(n_crops, H, T, dtype=torch.long)
            perms[c] = perm
        else:
            raise ValueError(fam)
        qkv[c, :, :3 * W] = torch.cat([q.reshape(T, W), k.reshape(T, W), v.reshape(T, W)], 1)
    return qkv.reshape(n_crops * T, ld).to(dtype), perms


def _heads(qkv, n_crops, T, W, H):
    """-> q, k, v float64 [n_crops, H, T, 64] from the input bits."""
    x = qkv[:, :3 * W].double().reshape(n_crops, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def _rows(x):
    """[n_crops, H, T, 64] -> [n_crops * T, H * 64]"""
    n, H, T, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * T, H * 64)


# ------------------------------------------------------------------------------------------------------------------- reference
def reference(qkv, n_crops, T, W, H):
    """float64 softmax(q k^T / 8) v of the given fp16 / fp32 input bits.  -> (want, A) [n_crops * T, W] float64, A = softmax(...) |v|:
    the weighted sum of absolute values, which every rounding error of the accumulation is proportional to."""
    q, k, v = _heads(qkv, n_crops, T, W, H)
    want, A = torch.empty_like(q), torch.empty_like(q)
    for c in range(n_crops):
        p = torch.softmax(q[c] @ k[c].transpose(-1, -2) * 0.125, dim=-1)
        want[c] = p @ v[c]
        A[c] = p @ v[c].abs()
    return _rows(want), _rows(A)


def _vmax(qkv, n_crops, T, W, H):
    v = _heads(qkv, n_crops, T, W, H)[2]
    return _rows(v.abs().amax(dim=(2, 3), keepdim=True).expand_as(v))


def bound_f16(qkv, n_crops, T, W, H, want, A, s=1.0):
    """Per-element bound of |got - want| for the fp16 kernels (k_attention_f16, k_attention_f16_long), derived from their arithmetic:

        s (2^-10 A + 2^-11 |want|) + T 2^-24 max|v| + 2^-25          (max|v| over the item's (crop, head) values)

      2^-11 A        the probabilities are rounded to fp16 before the second MFMA while their sum is taken before the rounding:
                     relative 2^-11 on every term of sum_k p_k v_k
      2^-11 A        the logits are fp32 sums of exact fp16 products and the exponent's argument fma(s, c2, -mx c2) is rounded in
                     fp32 at magnitudes up to ~300 (2^-24 * 300 = 2e-5 relative on p), the hardware exp2 adds ~1e-7, the online
                     kernel's alpha products a few 2^-24 per block: together far below 2^-11; the term is rounded up to it
      2^-11 |want|   the output is rounded to fp16
      T 2^-24 max|v| fp16-subnormal probabilities (absolute 2^-25 each against a row maximum of 1 -- after the division by the row
                     sum >= 1 at most that) and the fp32 accumulation of T terms
      2^-25          an fp16-subnormal output
    `s` is a safety factor on the relative terms; it stays 1 unless the hardware shows otherwise and may not exceed 2."""
    assert 1.0 <= s <= 2.0
    return s * (2 * U16 * A + U16 * want.abs()) + T * U32 * _vmax(qkv, n_crops, T, W, H) + 2.0 ** -25


def bound_f32(qkv, n_crops, T, W, H, want, A, s=1.0):
    """Per-element bound of |got - want| for k_attention_f32, u = 2^-24, following the kernel's own order of operations:

      logits     q is scaled by 0.125 first (exact), then one fmaf chain over d = 0 .. 63 per (row, key): the product of feature d
                 passes through 64 - d roundings, so |error| <= u/(1 - 64u) 0.125 sum_d (64 - d) |q_d k_d| =: e(row, key), and
                 eps_logit(row) = max_key e  (c = 64 - d per term: at most 64, 32.5 on average)
      exponent   the subtraction P - mx rounds once at |P - mx| <= 2 max_key |logit| =: R, expf is within 2 ulp:
                 every probability carries a relative error delta = eps_logit + u R + 2u (the error of mx itself cancels: softmax is
                 shift-invariant)
      numerator  sum_k p_k v_k as one fmaf chain over the T keys: T u relative to A, plus delta A from the probabilities
      row sum    per lane ceil(T / 64) terms, then six butterfly steps: (ceil(T / 64) + 6) u relative, plus delta; the division: u

        |got - want| <= s ((delta + T u) A + (delta + (ceil(T / 64) + 7) u) |want|) + T 2^-126 max|v|

    (the last term: probabilities that underflow).  With the logit term written as 2 eps_logit A this is the shape of the fp16 bound
    with fp32 round-off.  On 'gauss' it is more than 10 times tighter than bound_f16; on 'hot' the logits are 12 times larger and so is
    eps_logit."""
    assert 1.0 <= s <= 2.0
    q, k, v = _heads(qkv, n_crops, T, W, H)
    wd = torch.arange(64, 0, -1, dtype=torch.float64)                  # 64 - d roundings for feature d
    delta = torch.empty(n_crops, H, T, 1, dtype=torch.float64)
    for c in range(n_crops):
        e = (q[c].abs() * wd) @ k[c].abs().transpose(-1, -2) * 0.125 * (U32 / (1 - 64 * U32))
        R = 2 * (q[c] @ k[c].transpose(-1, -2) * 0.125).abs().amax(-1, keepdim=True)
        delta[c] = e.amax(-1, keepdim=True) + U32 * R + 2 * U32
    delta = _rows(delta.expand_as(q))
    return s * ((delta + T * U32) * A + (delta + ((T + 63) // 64 + 7) * U32) * want.abs()) + T * 2.0 ** -126 * _vmax(qkv, n_crops, T, W, H)


# ------------------------------------------------------------------------------------------------------------------- checker
def guarded_out(n_rows, W, dtype, device):
    """`out` for a launch: n_rows + 2 rows, NaN throughout, a row of GUARD before and after.  The kernel gets `out[1:]`."""
    buf = torch.full((n_rows + 2, W), float('nan'), dtype=dtype, device=device)
    buf[0] = GUARD
    buf[-1] = GUARD
    return buf


def check(buf, want, bnd, n_crops, T, q_tiles=None, what=''):
    """buf: the guarded_out buffer after the launch.  Asserts: both guard rows untouched; rows >= 32 q_tiles of every crop still NaN
    (q_tiles None: every row computed); every computed element finite and within `bnd` of `want`.
    -> the largest |got - want| / bnd over the computed elements."""
    buf = buf.detach().cpu()
    W = buf.shape[1]
    assert buf.shape[0] == n_crops * T + 2, (buf.shape, n_crops, T)
    assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), f'{what}: a guard row around out was written'
    got = buf[1:-1].double().reshape(n_crops, T, W)
    rows = T if q_tiles is None else min(T, 32 * q_tiles)
    if rows < T:
        assert bool(torch.isnan(got[:, rows:]).all()), f'{what}: rows beyond query tile {q_tiles} were written'
    got = got[:, :rows]
    assert bool(torch.isfinite(got).all()), f'{what}: {int((~torch.isfinite(got)).sum())} computed elements are not finite'
    ratio = (got - want.reshape(n_crops, T, W)[:, :rows]).abs() / bnd.reshape(n_crops, T, W)[:, :rows]
    worst = ratio.max().item()
    assert worst <= 1.0, f'{what}: |got - want| is {worst:.3f} of the bound at {tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape))}'
    return worst


def check_onehot(buf, qkv, perm, n_crops, T, W, H, crops=None):
    """'onehot' crops: out row = v[perm[row]] to fp16: |got - v| <= 2^-11 |v| + 2^-25 per element."""
    v = _heads(qkv, n_crops, T, W, H)[2]
    got = buf.detach().cpu()[1:-1].double().reshape(n_crops, T, H, 64).permute(0, 2, 1, 3)
    for c in (range(n_crops) if crops is None else crops):
        want = torch.gather(v[c], 1, perm[c][:, :, None].expand(H, T, 64))
        assert bool(((got[c] - want).abs() <= U16 * want.abs() + 2.0 ** -25).all()), f'crop {c}: a row is not the value row of its key'


# ------------------------------------------------------------------------------------------------------------------- emulation
def emulate(qkv, n_crops, T, W, H, blk=None, fault=None, fault_block=0):
    """The fp16 kernels' rounding on the CPU (numpy fp32): logits as fp32 sums of the fp16 products, p = exp2(fma(s, c2, -mx c2)) in fp32,
    row sum of the unrounded p, p rounded to fp16 for the second product, fp32 accumulation, fp16(o / sum).  blk None: one pass over
    all keys (k_attention_f16); blk 64: online softmax over 64-key blocks with the running maximum and the alpha rescale
    (k_attention_f16_long).  -> [n_crops * T, W] float16.

    fault: the output a wrong kernel would give.
      'halfmax'  the maximum taken over the keys with (key & 4) == 0 only -- one lane half's keys: the cross-half shuffle left out --
                 and p clamped to the fp16 range
      'padsum'   the T_pad - T padded keys (logit 0) counted in the row sum: the key >= T mask left out (T_pad: T rounded up to the
                 kernel's key block, 32 or `blk`)
      'stale'    the 32 keys of block `fault_block` (K and V) taken from the previous item: a prefetch that read the wrong item
      'vswap'    keys j and j + 1 of V (not of K) exchanged in the 8-key group at 32 fault_block: a wrong key <-> register mapping
      'noalpha'  (blk only) the rescale by alpha left out for the accumulator at 64-key block `fault_block` + 1"""
    x = qkv[:, :3 * W].float().numpy().reshape(n_crops, T, 3, H, 64)
    c2 = np.float32(0.125 * 1.4426950408889634)
    out = np.empty((n_crops, T, H, 64), np.float16)
    kb_keys = blk or 32
    T_pad = (T + kb_keys - 1) // kb_keys * kb_keys
    for item in range(n_crops * H):
        c, h = divmod(item, H)
        q, k, v = (x[c, :, i, h].copy() for i in range(3))
        if fault == 'stale':
            pc, ph = divmod((item - 1) % (n_crops * H), H)
            lo, hi = 32 * fault_block, min(T, 32 * fault_block + 32)
            k[lo:hi], v[lo:hi] = x[pc, lo:hi, 1, ph], x[pc, lo:hi, 2, ph]
        if fault == 'vswap':
            j = 32 * fault_block
            v[[j, j + 1]] = v[[j + 1, j]]
        s = q @ k.T                                                    # [T rows, T keys] fp32
        msk = (np.arange(T) & 4) == 0
        if blk is None:
            mx = (s[:, msk] if fault == 'halfmax' else s).max(1, keepdims=True)
            with np.errstate(over='ignore'):
                p = np.exp2(s * c2 + (-mx * c2), dtype=np.float32)
            if fault == 'halfmax':
                p = np.minimum(p, np.float32(65504.0))
            l = p.sum(1, dtype=np.float32, keepdims=True)
            if fault == 'padsum':
                l = l + np.float32(T_pad - T) * np.exp2(-mx * c2, dtype=np.float32)
            o = p.astype(np.float16).astype(np.float32) @ v
        else:
            m = np.full((T, 1), -np.inf, np.float32)
            l = np.zeros((T, 1), np.float32)
            o = np.zeros((T, 64), np.float32)
            for b, k0 in enumerate(range(0, T, blk)):
                sb = s[:, k0:k0 + blk]
                mb = sb[:, msk[k0:k0 + blk]] if fault == 'halfmax' else sb
                mx = np.maximum(m, mb.max(1, keepdims=True))
                with np.errstate(over='ignore', invalid='ignore'):
                    alpha = np.exp2((m - mx) * c2, dtype=np.float32)
                    p = np.exp2(sb * c2 + (-mx * c2), dtype=np.float32)
                if fault == 'halfmax':
                    p = np.minimum(p, np.float32(65504.0))
                ps = p.sum(1, dtype=np.float32, keepdims=True)
                if fault == 'padsum' and k0 + blk > T:
                    ps = ps + np.float32(T_pad - T) * np.exp2(-mx * c2, dtype=np.float32)
                l = l * alpha + ps
                o = o * (np.float32(1.0) if fault == 'noalpha' and b == fault_block + 1 else alpha) + p.astype(np.float16).astype(np.float32) @ v[k0:k0 + blk]
                m = mx
        with np.errstate(over='ignore', invalid='ignore'):
            out[c, :, h] = (o / l).astype(np.float16)
    return torch.from_numpy(out.reshape(n_crops * T, W))


def as_guarded(out, q_tiles=None, T=None):
    """An emulated `out` [rows, W] in the guarded_out layout the checker takes (rows >= 32 q_tiles of every crop NaN)."""
    buf = guarded_out(out.shape[0], out.shape[1], out.dtype, 'cpu')
    buf[1:-1] = out
    if q_tiles is not None:
        buf[1:-1].reshape(-1, T, out.shape[1])[:, 32 * q_tiles:] = float('nan')
    return buf
