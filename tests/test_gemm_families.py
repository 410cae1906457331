"""Every kernel family of the projection GEMM (vg_gemm; csrc/vit.hip k_gemm_f16, k_gemm_f16_pp64, k_gemm_f16_w4, k_gemm_f32, k_gemm_f32_mfma)
with its plain epilogues against the float64 references of tests/gemm_ref.py, at the edges of the K pipelines and of the tile orders.

Every case names the family it is written for and first asks vg_gemm_family (the function vg_gemm's own dispatch asks) that this family
runs -- on the CPU too, over the whole table.  Then four input families go through vg_gemm (gemm_ref.operands):
  gauss    bounded per element by (c + 2) u S + the epilogue's own operations (gemm_ref.formula), fp16 outputs to one ulp beyond it, and up
           to K = 768 at least 0.99 of the elements whose bound is below a quarter ulp correctly rounded
  integer  every partial sum exact in fp32 in any order: epilogues 0, 2, 3, 4 bit for bit, 1 within its QuickGELU term plus one fp16 ulp
  onehot   output (m, n) names one (n, k): bit for bit; together the (a, s) of a shape name every k
  guarded  gauss, every operand a view inside a larger NaN-filled allocation: results within bound, every guard byte of C and resid intact
The worst err / bound, the exact fraction and the qualifying share are printed per case (pytest -s)."""
import functools

import pytest
import torch

import gemm_ref as G

VG_OK, VG_ERR_ARG = 0, 1
ENV = {'VG_GEMM_W4': '1', 'VG_GEMM_F32_MFMA': '1'}          # the defaults, set explicitly: the table does not depend on the caller's environment


def _cases():
    out = []

    def add(family, shapes, epis, **env):
        for shape in shapes:
            for epi in epis:
                out.append(pytest.param(family, shape, epi, tuple(sorted(env.items())),
                                        id='-'.join([family, 'x'.join(map(str, shape)), f'epi{epi}'] + [f'{k[3:].lower()}{v}' for k, v in sorted(env.items())])))
    # k_gemm_f16 (N % 256 == 128, or K % 64 == 32, or K == 64): 1, 2, 3, 4, 5, 7 K-steps of its 3-stage ring; 15 tiles (not a multiple of
    # 8 for xcd_remap); column chunks narrower than the row of tiles (ntn 9 -> cw 3)
    add('f16', [(256, 128, 32), (256, 128, 64), (256, 128, 96), (256, 128, 128), (256, 384, 160), (512, 128, 224), (768, 640, 96),
                (512, 1152, 1568)], (0, 1, 2, 3))
    # k_gemm_f16_pp64 (X ring 2, W ring 3): 2, 3, 4, 5, 7 K-tiles; ntn 10 (cw 2) and 11 (cw 1)
    add('pp64', [(256, 256, 128), (256, 256, 192), (256, 256, 256), (256, 512, 320), (512, 768, 448), (256, 2560, 128), (256, 2816, 128)],
        (0, 1, 2, 3, 4), VG_GEMM_W4='0')
    # ... and what k_gemm_f16_w4 hands over to it: fewer than four K-tiles, and the fp16 residual stream
    add('pp64', [(256, 256, 128), (256, 256, 192)], (0, 1, 2, 3, 4), VG_GEMM_W4='1')
    add('pp64', [(256, 256, 256)], (4,), VG_GEMM_W4='1')
    # k_gemm_f16_w4: 4 ... 9 K-tiles on ONE tile (the 8-workgroup minimum grid: seven idle workgroups); ntn 3, 10 (cw 2), 11 (cw 1)
    add('w4', [(256, 256, 64 * t) for t in range(4, 10)] + [(256, 768, 256), (256, 2560, 256), (256, 2816, 256)], (0, 1, 2, 3), VG_GEMM_W4='1')
    # fp32: the vector kernel, the MFMA kernel, and the MFMA kernel's shapes on the vector kernel
    add('f32', [(64, 64, 16), (192, 64, 48), (64, 192, 80)], (0, 1, 2, 3))
    add('f32_mfma', [(128, 128, 16), (256, 384, 32), (128, 128, 272)], (0, 1, 2, 3))
    add('f32', [(128, 128, 16), (256, 384, 32), (128, 128, 272)], (0, 1, 2, 3), VG_GEMM_F32_MFMA='0')
    return out


CASES = _cases()

# (dtype, epi-independent) shapes no kernel takes: one unit off a legal shape in M, N or K
REFUSED = {1: [(128, 256, 128), (384, 256, 128), (128, 256, 256), (384, 512, 256), (256, 192, 128), (256, 64, 32), (256, 128, 16), (256, 256, 144),
               (256, 128, 48)],
           0: [(32, 64, 16), (96, 64, 16), (64, 96, 16), (64, 32, 16), (64, 64, 8), (64, 64, 24), (128, 128, 8)]}
REFUSED_EPI4 = [(256, 128, 128), (256, 384, 128), (256, 256, 64), (256, 256, 96), (128, 256, 128), (384, 256, 256)]      # (dtype 1; dtype 0 refuses every shape)


def _set_env(monkeypatch, env):
    for k, v in {**ENV, **dict(env)}.items():
        monkeypatch.setenv(k, v)


def _probe(dtype, epi, shape):
    from vilgod_amd._lib import lib
    return lib.vg_gemm_family(dtype, epi, *shape)


def chunk_tiles(N, K):
    """gemm_chunk_tiles (k_gemm_f16): column tiles (128 wide) per chunk, <= 2.4 MB of weight rows."""
    ntn = N // 128
    cw_max = max(1, 2400000 // (128 * K * 2))
    if cw_max >= ntn:
        return ntn
    nchunks = -(-ntn // cw_max)
    while ntn % nchunks:
        nchunks += 1
    return ntn // nchunks


def chunk_tiles_256(ntn):
    """gemm_chunk_tiles_256 (the 256 x 256 kernels)."""
    if ntn <= 9:
        return ntn
    cw = 4
    while ntn % cw:
        cw -= 1
    return cw


# ------------------------------------------------------------------------------------------------------------------- the probe (CPU)
@pytest.mark.parametrize('family,shape,epi,env', CASES)
def test_probe_names_the_family_of_every_case(family, shape, epi, env, monkeypatch):
    _set_env(monkeypatch, env)
    assert _probe(G.family_dtype(family), epi, shape) == G.FAMILY_CODES[family]


def test_probe_follows_the_switches_and_refuses_what_vg_gemm_refuses(monkeypatch):
    _set_env(monkeypatch, {})
    assert _probe(1, 0, (256, 256, 256)) == G.FAMILY_CODES['w4']            # four K-tiles: the shortest loop k_gemm_f16_w4 takes
    assert _probe(1, 0, (256, 256, 192)) == G.FAMILY_CODES['pp64']
    assert _probe(1, 0, (256, 256, 64)) == G.FAMILY_CODES['f16']            # one K-tile: neither 256 x 256 kernel
    assert _probe(0, 0, (128, 128, 16)) == G.FAMILY_CODES['f32_mfma']
    assert _probe(0, 0, (128, 192, 16)) == G.FAMILY_CODES['f32']            # N % 128 != 0
    for w4 in ('0', '1'):
        monkeypatch.setenv('VG_GEMM_W4', w4)
        for dtype, shapes in REFUSED.items():
            for shape in shapes:
                for epi in range(4):
                    assert _probe(dtype, epi, shape) < 0, (dtype, epi, shape)
        for shape in REFUSED_EPI4:
            assert _probe(1, 4, shape) < 0, shape
        assert _probe(0, 4, (256, 256, 256)) < 0
        for epi in (-1, 5, 6):
            assert _probe(1, epi, (256, 256, 256)) < 0


def test_the_table_reaches_the_chunked_tile_orders():
    assert chunk_tiles(1152, 1568) == 3 < 1152 // 128                      # k_gemm_f16: cw < ntn
    assert chunk_tiles(640, 96) == 5 and (768 // 256) * 5 % 8 != 0          # 15 tiles: xcd_remap's remainder
    assert chunk_tiles_256(10) == 2 and chunk_tiles_256(11) == 1 and chunk_tiles_256(3) == 3


def test_onehot_shifts_name_every_k():
    for p in CASES:
        family, (M, N, K), _, _ = p.values
        hit = torch.zeros(K, dtype=torch.bool)
        for a, s in G.onehot_params(M, K):
            hit[(a * torch.arange(M) + s) % K] = True
        assert hit.all(), (family, M, N, K)


# ------------------------------------------------------------------------------------------------------------------- the checkers (CPU)
SMALLEST = {'f16': [(256, 128, 32), (256, 128, 96)], 'pp64': [(256, 256, 128)], 'w4': [(256, 256, 256)], 'f32': [(64, 64, 16)],
            'f32_mfma': [(128, 128, 16)]}


def _epis(family):
    return (0, 1, 2, 3, 4) if family == 'pp64' else (0, 1, 2, 3)


def _applies(fault, family, epi):
    if fault == 'trunc':
        return G.family_dtype(family) == 1 and epi in (0, 1, 4)
    if fault == 'gelu17':
        return epi == 1
    if fault == 'resid_twice':
        return epi in (2, 4)
    if fault == 'bias_shift':
        return epi != 3
    return True


@pytest.mark.parametrize('family', list(SMALLEST))
def test_checkers_accept_the_emulated_kernel_and_reject_synthesised_faults(family):
    """The checkers have teeth, without running a broken kernel: a float32 emulation of a correct kernel of the family (gemm_ref.emulate)
    passes every input family and epilogue on the smallest shapes; each synthesised fault is rejected by at least one check there."""
    dtype = G.family_dtype(family)
    caught = {f: [] for f in G.FAULTS}
    for shape in SMALLEST[family]:
        for kind in G.KINDS:
            o = G.operands(kind, *shape, dtype, *((65, 3) if kind == 'onehot' else ()))
            for epi in _epis(family):
                G.check_case(G.emulate(o, epi, family), o, epi, family)
                for fault in G.FAULTS:
                    if not _applies(fault, family, epi):
                        continue
                    try:
                        G.check_case(G.emulate(o, epi, family, fault), o, epi, family)
                    except AssertionError:
                        caught[fault].append((shape, kind, epi))
    for fault, where in caught.items():
        if not any(_applies(fault, family, epi) for epi in _epis(family)):
            continue                                # (an fp32 kernel has no fp16 output to truncate)
        assert where, f'{family}: no check rejects {fault}'
    # the faults that move an fp16 output by less than its bound are the exactness clause's; the exact families see every dropped element
    assert any(kind == 'integer' for _, kind, _ in caught['drop_k']) and any(kind == 'onehot' for _, kind, _ in caught['swap_runs'])
    print(family, {f: len(w) for f, w in caught.items()})


def test_guard_check_sees_one_changed_byte():
    g = G.Guarded(torch.zeros(4, 8, dtype=torch.float16), 'cpu')
    assert g.intact() and g.view.shape == (4, 8) and g.pad == G.GUARD_ROWS * 8
    g.view.fill_(1.0)
    assert g.intact()
    g.buf[g.pad - 1] = 0.0
    assert not g.intact()
    g = G.Guarded(torch.zeros(16), 'cpu')
    g.buf[-1] = float('inf')
    assert not g.intact()


def test_round16_is_one_correct_rounding():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -11, 2047.5, 2049.0, 2049.0 + 2.0 ** -30, 3e-8, -65504.0, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, 2048.0, 2048.0, 2050.0, 2.0 ** -24, -65504.0, 0.0], dtype=torch.float64)
    assert torch.equal(G.round16(v), want)
    x = torch.randn(4096, dtype=torch.float32, generator=G.gen('round16'))
    assert torch.equal(G.round16(x.double()), x.half().double())           # (a float rounds to half in one step)


# ------------------------------------------------------------------------------------------------------------------- the kernels (GPU)
@functools.lru_cache(maxsize=12)
def _operands(kind, M, N, K, dtype, a=1, s=0):
    """One reference per (input family, shape), shared by the epilogues of the shape (never modified)."""
    return G.operands(kind, M, N, K, dtype, a, s)


def _launch(o, epi, dtype, cuda, guarded=False):
    """vg_gemm on the operands -> (status, output on the CPU, untouched).  Outputs the epilogue does not write are passed NaN-filled and
    `untouched` says they still are; with `guarded`, also that every guard byte of C and resid holds its fill pattern."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    M, N, K = o.shape
    nan = float('nan')
    c_dtype = torch.float32 if (epi == 3 or dtype == 0) else torch.float16
    C0 = torch.full((M, N), nan, dtype=c_dtype)
    R0 = o.resid16 if epi == 4 else o.resid if epi == 2 else torch.full((M, N), nan)
    tensors = [o.X, o.W, o.bias, C0, R0]
    if guarded:
        guards = [G.Guarded(t, cuda) for t in tensors]
        X, W, b, C, R = (g.view for g in guards)
    else:
        guards = []
        X, W, b, C, R = (t.to(cuda).clone() for t in tensors)
    rc = lib.vg_gemm(dtype, epi, ptr(X), ptr(W), ptr(b), ptr(C), ptr(R), M, N, K, stream_ptr())
    torch.cuda.synchronize()
    out, other = (R, C) if epi in (2, 4) else (C, R)
    untouched = G.all_nan_fill(other) and all(g.intact() for g in guards[3:])
    if guarded:
        untouched = untouched and bool(torch.equal(X.cpu(), o.X) and torch.equal(W.cpu(), o.W) and torch.equal(b.cpu(), o.bias))
    return rc, out.cpu(), untouched


@pytest.mark.gpu
@pytest.mark.parametrize('family,shape,epi,env', CASES)
def test_family_against_float64(cuda, family, shape, epi, env, monkeypatch):
    _set_env(monkeypatch, env)
    dtype = G.family_dtype(family)
    assert _probe(dtype, epi, shape) == G.FAMILY_CODES[family]
    M, N, K = shape
    runs = [('gauss', (), False), ('integer', (), False)] + [('onehot', p, False) for p in G.onehot_params(M, K)] + [('gauss', (), True)]
    for kind, p, guarded in runs:
        o = _operands(kind, M, N, K, dtype, *p)
        rc, out, untouched = _launch(o, epi, dtype, cuda, guarded)
        assert rc == VG_OK, rc
        name = 'guarded' if guarded else kind + ''.join(f'_{v}' for v in p)
        try:
            ratio, frac, share = G.check_case(out, o, epi, family)
        except AssertionError as e:
            raise AssertionError(f'{family} {shape} epi {epi} {name}: {e}') from None
        assert untouched, f'{family} {shape} epi {epi} {name}: an output the epilogue does not own, an operand or a guard byte was written'
        fmt = lambda v: '-' if v is None else f'{v:.4f}'        # noqa: E731
        print(f'GEMMFAM family={family} shape={M}x{N}x{K} epi={epi} kind={name} err/bound={ratio:.4f} exact={fmt(frac)} share={fmt(share)}')


@pytest.mark.gpu
@pytest.mark.parametrize('w4', ['0', '1'])
def test_refused_shapes_write_nothing(cuda, w4, monkeypatch):
    """One unit off a legal shape in M, N or K, epilogue 4 on fp32 operands or without a 256 x 256 kernel: VG_ERR_ARG, the probe negative,
    every byte of the NaN-prefilled outputs kept."""
    from vilgod_amd._lib import lib, ptr, stream_ptr
    _set_env(monkeypatch, {'VG_GEMM_W4': w4})
    nan = float('nan')
    ops = {1: torch.zeros(512 * 512, dtype=torch.float16, device=cuda), 0: torch.zeros(512 * 512, device=cuda)}
    bias = torch.zeros(512, device=cuda)
    todo = [(dtype, epi, shape) for dtype, shapes in REFUSED.items() for shape in shapes for epi in range(4)]
    todo += [(1, 4, shape) for shape in REFUSED_EPI4] + [(0, 4, (256, 256, 256)), (1, 5, (256, 256, 256)), (1, -1, (256, 256, 256))]
    for dtype, epi, shape in todo:
        M, N, K = shape
        C = torch.full((512 * 512,), nan, device=cuda)
        R = torch.full((512 * 512,), nan, device=cuda)
        assert _probe(dtype, epi, shape) < 0, (dtype, epi, shape)
        assert lib.vg_gemm(dtype, epi, ptr(ops[dtype]), ptr(ops[dtype]), ptr(bias), ptr(C), ptr(R), M, N, K, stream_ptr()) == VG_ERR_ARG, (dtype, epi, shape)
        torch.cuda.synchronize()
        assert G.all_nan_fill(C) and G.all_nan_fill(R), (dtype, epi, shape)
