"""The L-shape box kernels (csrc/lshape.hip: k_lshape_score, k_lshape_pick) at their argument and size edges, through vg_cluster_lshape.

The bars (tests/lshape_edges_ref.py states and derives them):
  box, aux[2]   bit for bit the restatement `pick_box` at the index the kernel reports
  criteria      closeness within (n + 1) 2^-53 of math.fsum of the correctly rounded terms; variance within
                (max(n_x, n_y) + 6) 2^-53 |exact| + (1 + 2^-20) 2^-106 (n_x^2 mu_x^2 + n_y^2 mu_y^2) of the rational value
  index         the first index of the exact maximum wherever that maximum leads by more than the two bounds; else among the close ones
                (such clusters are counted: at most 1 % of a family, none on the fixture); and always the first maximum of the
                kernel's own criteria, whose value is aux[1]
No other tolerance is used below, except where the restatement is pinned to the recorded reference outputs, at the tolerances of
tests/test_lshape.py (1e-6 closeness, 1e-9 variance): the recording used numpy's dot, whose rounding is the host's.

CPU: fma32 / fma64 against rational arithmetic; the restatement against the fixture; the numpy emulation of the kernels' order inside
     both bounds on every input of this file; every synthesised fault of lshape_edges_ref.FAULTS rejected by a named case; the share of
     ambiguous clusters from the exact criteria alone.
GPU: tables built here (exact ties from row k on, A = 1 .. 9001), sizes 0 .. 1025 with each extreme point at each position, gathered
     lists at strides 3, 4, 5, 7 with shared points, decisions at equality, the clamp at and next to delta_zero, five families, the
     wrapper, and two runs of everything giving the same bytes.

Measured (printed under -s):
  restatement against the fixture   closeness: 0 of 768 float32 values (corners, centre, l, w of 64 clusters) differ in bits from the
                                    recording; variance: 6 of 768 float64 values differ, by 1 ulp each (numpy's dot on the recording host)
  share of the criterion bound      the emulation and the kernel on an MI355X use the same shares, group by group:
                                    closeness  tie 0.239, sizes 0.292, index 0.394, clamp 0.285, fixture 0.076, real 0.088, seeded 0.340,
                                               delta 1: 0.333, delta 0.5: 0.141
                                    variance   tie 0.195, sizes 0.079, index 0.288, fixture 0.176, real 0.215, seeded 0.321,
                                               delta 0.5: 0.359, delta 0.01: 0.160
                                    (the equality cases: 0, their sums are exact)
  ambiguous clusters                0 in every family and group (fixture 64, real 18, seeded 210, deltas 60 / 60 / 12 clusters)
The exact variance criteria of the families take the CPU some seconds (the 20 000-point fixture cluster at 901 angles most of them); they
are computed once per process and shared by the CPU and GPU tests.
"""
import ctypes

import numpy as np
import pytest

import lshape_edges_ref as E

CRITS = [E.CLOSENESS, E.VARIANCE]
IDS = ['closeness', 'variance']
AMBIGUOUS_CAP = 0.01


GROUP_CRITS = [(g, c) for g in E.GROUPS for c in CRITS if not (g == 'clamp' and c == E.VARIANCE)]
GROUP_IDS = [f'{g}-{IDS[c]}' for g, c in GROUP_CRITS]


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_fma_restatements_round_once():
    """fma32 and fma64 against rational arithmetic: random operands, sums that cancel, and products half an ulp from a tie."""
    rng = np.random.default_rng(0)
    n = 3000
    a, b = rng.uniform(-60, 60, n), rng.uniform(-1, 1, n)
    c = np.where(rng.random(n) < 0.5, -a * b * (1 + rng.integers(-3, 4, n) * 2.0 ** -rng.integers(20, 60, n)), rng.uniform(-60, 60, n))
    c[::7] *= 2.0 ** -30
    got = E.fma64(a, b, c)
    assert all(got[i] == E.fma_exact(a[i], b[i], c[i], np.float64) for i in range(n))
    a32, b32, c32 = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    c32[::5] = (a32[::5].astype(np.float64) * b32[::5]).astype(np.float32) * np.float32(2.0 ** 24)      # far above the product
    got = E.fma32(a32, b32, c32)
    assert got.dtype == np.float32
    assert all(got[i] == E.fma_exact(a32[i], b32[i], c32[i], np.float32) for i in range(n))
    naive = (a * b + c)
    print(f'fma64 differs from the two-rounding a * b + c on {int((naive != E.fma64(a, b, c)).sum())} of {n} samples')


def test_exact_column_sums_match_integer_arithmetic():
    """colsum_int (float64 passes whose sums are exact) against Python integers, over 68 binades and 1 .. 5000 rows; so is the sum of
    squares from the three exact products of the 26-bit halves."""
    rng = np.random.default_rng(0)
    for n in (1, 3, 100, 5000):
        X = rng.uniform(-1, 1, (n, 40)) * 2.0 ** rng.integers(-60, 8, (n, 40))
        X[rng.random((n, 40)) < 0.3] = 0
        low = E._low_bit(X)
        ints = E._to_int(np.abs(X), low) * np.sign(X).astype(np.int64).astype(object)
        assert E.colsum_int(X, low).tolist() == ints.sum(axis=0).tolist()
        hi, lo = E._split(X)
        S2 = E.colsum_int(hi * hi, 2 * low) + 2 * E.colsum_int(hi * lo, 2 * low) + E.colsum_int(lo * lo, 2 * low)
        assert S2.tolist() == (ints * ints).sum(axis=0).tolist()


def _ulps(a, b, dtype):
    it = {np.float32: np.int32, np.float64: np.int64}[dtype]
    a, b = (np.ascontiguousarray(v, dtype).view(it).astype(np.int64) for v in (a, b))
    return np.abs(a - b)


@pytest.mark.parametrize('crit', CRITS, ids=IDS)
def test_restatement_reproduces_the_fixture(golden_dir, crit):
    """pick_box at the recorded index against the recorded corners, angle and box, at the tolerances tests/test_lshape.py uses; the
    values that differ in bits are the effect of numpy's dot on the recording host (printed)."""
    g = np.load(f'{golden_dir}/lshape_golden.npz')
    key, tol = ('closeness', 1e-6) if crit == E.CLOSENESS else ('variance', 1e-9)
    table, T = E.angle_table(crit), E.dtype_of(crit)
    differ, worst, total = 0, 0, 0
    for c, p in enumerate(E.fixture_clusters(golden_dir)):
        k = int(g[f'{key}_index'][c])
        box, aux2, corners = E.pick_box(p, table[k], crit)
        assert aux2 == g[f'{key}_angle'][c], c
        assert np.allclose(corners, g[f'{key}_corners'][c], rtol=0, atol=tol), c
        assert np.allclose(box, g[f'{key}_box'][c], rtol=0, atol=tol), c
        assert np.array_equal(box[[2, 5, 6]], g[f'{key}_box'][c][[2, 5, 6]]), c           # cz, h + 0.3 and rz involve no dot
        mine, theirs = np.r_[corners.ravel(), box[[0, 1, 3, 4]]], np.r_[g[f'{key}_corners'][c].ravel(), g[f'{key}_box'][c][[0, 1, 3, 4]]]
        d = _ulps(mine, theirs, T)
        differ, worst, total = differ + int((d > 0).sum()), max(worst, int(d.max())), total + d.size
    print(f'{key}: {differ} of {total} {T.__name__} values differ in bits from the recording, by at most {worst} ulp')


@pytest.mark.parametrize('group,crit', GROUP_CRITS, ids=GROUP_IDS)
def test_emulation_is_inside_the_bounds(golden_dir, group, crit):
    """The emulation of a correct kernel passes every check on every input of this file; its worst share of the criterion bound is
    printed.  The share of ambiguous clusters comes from the exact criteria alone."""
    share, ambiguous, clusters = 0.0, 0, 0
    for case in E.cases(group, crit, golden_dir):
        for xyz, ex, inv in E.reference(case):                        # before any kernel output: who is ambiguous?
            if ex is not None:
                clusters += 1
                ambiguous += E.decide(ex, inv)[0] is None
    print(f'{group} {IDS[crit]}: {ambiguous} ambiguous of {clusters} clusters')
    assert ambiguous <= (0 if group in ('family/fixture', 'tie', 'equal', 'clamp') else AMBIGUOUS_CAP * clusters)
    for case in E.cases(group, crit, golden_dir):
        share = max(share, E.check(case, *E.emulate(case))['share'])
    print(f'{group} {IDS[crit]}: the emulation uses {share:.3f} of the criterion bound')
    assert share <= 1.0


def _first(cases_, pred):
    return next(c for c in cases_ if pred(c))


def test_checker_accepts_the_emulated_kernels_and_rejects_synthesised_faults(golden_dir):
    """Each wrong kernel is rejected by the named case(s); the same cases accept the emulation of the right one."""
    C, V = E.CLOSENESS, E.VARIANCE
    tie = lambda crit, A, k: _first(E.cases('tie', crit), lambda c: c['name'].endswith(f'/A{A}/k{k}'))
    sizes = [E.cases('sizes', C)[0], E.cases('sizes', V)[0]]
    eq = lambda crit, tag: _first(E.cases('equal', crit), lambda c: c['name'].endswith(tag))
    clamp = E.cases('clamp', C)
    idx = lambda crit, s: _first(E.cases('index', crit), lambda c: c['name'].endswith(f'stride{s}'))
    small = E.make_case('teeth/fixture-head', E.fixture_clusters(golden_dir)[:12], C, E.angle_table(C))
    named = {
        'zero_start_score': sizes,                                    # min / max started from 0, in either kernel
        'zero_start_pick': sizes,
        'flip_le': [eq(C, 'honest'), eq(V, 'honest')],
        'swap_ge': [eq(C, 'same-axes'), eq(V, 'same-axes')],
        'side_le': [eq(V, 'sides')],
        'clamp_dropped': clamp[:1] + clamp[-1:],
        'clamp_f32': [c for c in clamp if c['name'].endswith(('passed0.01', 'passed0.05', 'passed1e-06'))],      # (a delta_zero that is no float32 value)
        'acc_f32': [small, sizes[1]],
        'last_max': [tie(C, 5, 0), tie(V, 257, 64)],
        'wave_tie_high': [tie(C, 257, 63), tie(V, 513, 64)],          # rows 63.. tie: waves 0 (63) and 1 (64) both hold the maximum;
                                                                      # (with k = 0 every thread's start, angle 0, already wins)
        'loop_256': [tie(C, 257, 256), tie(V, 513, 256), tie(V, 9001, 9000)],
        'rz_unflipped': [eq(C, 'honest'), eq(V, 'same-axes')],
        'f64_lw': [small],                                            # l and w from float32 corners, in float64
        'f64_centre': [small],
        'index_ignored': [idx(C, 3), idx(V, 5)],
        'stride3': [idx(C, 4), idx(V, 7)],
    }
    assert set(named) == set(E.FAULTS)
    for fault, cases_ in named.items():
        for case in cases_:
            E.check(case, *E.emulate(case))
            assert E.rejected(case, E.emulate(case, fault)), f'{fault} is accepted on {case["name"]}'
    # the checker's own structure: a work row that is off by two bounds, an index that is not the first maximum, one flipped box bit
    case = small
    box, aux, work = E.emulate(case)
    w2 = work.copy()
    w2[3, 7] *= 1 + 2 * (len(E.gather(case, 3)) + 1) * E.U
    assert E.rejected(case, (box, aux, w2))
    a2 = aux.copy()
    a2[0, 0] += 1
    assert E.rejected(case, (box, a2, work))
    b2 = box.copy()
    b2.view(np.uint64)[5, 3] ^= 1
    assert E.rejected(case, (b2, aux, work))
    a3 = aux.copy()
    a3.view(np.uint64)[5, 2] ^= 1
    assert E.rejected(case, (box, a3, work))


def test_designed_cases_are_what_they_claim():
    """The clamp cases hold beta one float32 step below, at and above float32(delta_zero); the tie tables' rows from k on are equal in
    columns 0..3 and distinct in 4..7; the size cases place every extreme point where the label says."""
    for case in E.cases('clamp', E.CLOSENESS):
        dz32 = np.float32(float(case['name'].split('dz')[1].split('/')[0]))
        dx, dy = E.distances(E.gather(case, 3)[:, :2], case['table'][:1], E.CLOSENESS)
        beta = np.minimum(dx, dy)[4:, 0]
        assert beta[1] == dz32 and beta[0] == np.nextafter(dz32, np.float32(0)) and beta[2] == np.nextafter(dz32, np.float32(100))
        assert (beta[1].astype(np.float64) == case['dz']) == (case['dz'] == float(dz32))
    for A in E.TIE_A:
        for k in E.tie_ks(A):
            t = E.tie_case(E.VARIANCE, A, k)['table']
            assert len(np.unique(t[k:, :4], axis=0)) == 1 and len(np.unique(t[:, 4])) == A
            assert k == 0 or (len(np.unique(t[:k, :4], axis=0)) == 1 and not np.array_equal(t[0, :4], t[k, :4]))
    case, labels = E.size_case(E.CLOSENESS)
    assert sorted({len(E.gather(case, c)) for c in range(len(labels))}) == sorted(E.SIZES)
    seen = set()
    for c, label in enumerate(labels):
        if '@' not in label:
            continue
        xy = E.gather(case, c)[:, :2]
        e, pos = int(label.split('extreme')[1][0]), label.split('@')[1]
        where = [int(np.argmin(xy[:, 0])), int(np.argmax(xy[:, 0])), int(np.argmin(xy[:, 1])), int(np.argmax(xy[:, 1]))][e]
        assert where == {'first': 0, 'last': len(xy) - 1}.get(pos, int(pos) if pos.isdigit() else None), label
        seen.add((e, pos))
    assert seen == {(e, str(p)) for e in range(4) for p in E.POSITIONS}


# ------------------------------------------------------------------------------------------------------------------- GPU
def _launch(cuda, case):
    """vg_cluster_lshape on a case -> (box [C, 7], aux [C, 3], work [C, A]) numpy; the outputs start as NaN"""
    import torch
    from vilgod_amd._lib import lib, ptr, check
    d_X = torch.from_numpy(case['pts']).to(cuda)
    d_index = torch.from_numpy(case['index']).to(cuda)
    d_seg = torch.from_numpy(case['seg']).to(cuda)
    tab = torch.from_numpy(case['table']).to(cuda)
    C, A = len(case['seg']) - 1, len(case['table'])
    work, box, aux = (torch.full((C, k), float('nan'), dtype=torch.float64, device=cuda) for k in (A, 7, 3))
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.vg_cluster_lshape(ptr(d_X), d_X.stride(0), ptr(d_index), ptr(d_seg), C, case['crit'], ptr(tab), A, case['dz'], ptr(work),
                                ptr(box), ptr(aux), stream), 'vg_cluster_lshape')
    torch.cuda.synchronize(cuda)
    return box.cpu().numpy(), aux.cpu().numpy(), work.cpu().numpy()


def _run_twice(cuda, case):
    out, again = _launch(cuda, case), _launch(cuda, case)
    for a, b in zip(out, again):
        assert a.tobytes() == b.tobytes(), f'{case["name"]}: two runs differ'
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('group,crit', GROUP_CRITS, ids=GROUP_IDS)
def test_hip_lshape_edges(cuda, golden_dir, group, crit):
    """Every case of the group through the entry point, twice, held to every bar."""
    share, ambiguous, clusters = 0.0, 0, 0
    for case in E.cases(group, crit, golden_dir):
        out = _run_twice(cuda, case)
        r = E.check(case, *out)
        share, ambiguous, clusters = max(share, r['share']), ambiguous + r['ambiguous'], clusters + r['clusters']
        if group == 'index':                                          # the same bits as the packed form
            for a, b in zip(out, _launch(cuda, E.packed(case))):
                assert a.tobytes() == b.tobytes(), case['name']
    print(f'{group} {IDS[crit]}: the kernel uses {share:.3f} of the criterion bound; {ambiguous} ambiguous of {clusters} clusters')


@pytest.mark.gpu
def test_hip_lshape_empty_cluster_between_neighbours(cuda):
    """n = 0 between two clusters: seven NaNs, aux {0, 0.0, NaN}, an all-zero work row; the neighbours as if it were not there."""
    for crit in CRITS:
        case = E.cases('sizes', crit)[0]
        cl = [E.gather(case, c) for c in (2, 3, 4)]
        assert [len(p) for p in cl] == [3, 0, 63]
        box, aux, work = _launch(cuda, E.make_case(f'empty/{IDS[crit]}', cl, crit, case['table']))
        assert np.isnan(box[1]).all() and aux[1, 0] == 0 and aux[1, 1] == 0 and np.isnan(aux[1, 2]) and not work[1].any()
        alone = _launch(cuda, E.make_case(f'empty/{IDS[crit]}/alone', [cl[0], cl[2]], crit, case['table']))
        for got, want in zip((box, aux, work), alone):
            assert got[[0, 2]].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_hip_lshape_wrapper_returns_the_entry_points_bits(cuda):
    """PseudoLabelPipeline.fit_boxes(method={name, args}) with a delta and delta_zero of the caller's, in both box modes."""
    import torch
    from vilgod_amd.pipeline import PseudoLabelPipeline
    cl = E.seeded_clusters(30, 23)
    for crit, args in ((E.CLOSENESS, {'delta': 3, 'delta_zero': 0.05}), (E.VARIANCE, {'delta': 0.7})):
        case = E.gathered(E.make_case(f'wrapper/{IDS[crit]}', cl, crit, E.angle_table(crit, **args), dz=args.get('delta_zero', 1.0)), 5, 9)
        out = _launch(cuda, case)
        E.check(case, *out)
        want = out[0]
        d_X = torch.from_numpy(case['pts']).to(cuda)
        pipe = PseudoLabelPipeline(device=cuda, max_points=len(case['pts']) + 16, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
        for mode in ('fast', 'reference'):
            pipe.box_mode = mode
            got = pipe.fit_boxes(d_X, case['index'], case['seg'], method={'name': E.NAMES[crit], 'args': args})
            assert got.tobytes() == want.tobytes(), (crit, mode)
