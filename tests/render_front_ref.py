"""Shared by tests/test_render_front.py and tests/test_render.py: the renderer's front end (k_gather_ego, k_cluster_median's view angle
and rotation row, k_cluster_rot, k_to_origin of csrc/render.hip) restated in plain numpy, and the exact values those restatements are
themselves held to.  TEST INFRASTRUCTURE ONLY: it imports no kernel code and nothing from oracle/.

RESTATEMENTS (`gather_ego`, `view_rotation`, `to_origin`): elementwise numpy float64 in exactly the kernels' operation order.  They are
a bitwise bar for the kernels because render.hip is compiled with -ffp-contract=off (asserted in the test), numpy's elementwise float64
`+ - *` and the float32 `-` are single IEEE operations, and the float64 -> float32 conversion rounds to nearest even on both sides.  The
exception is the sine / cosine inside `view_rotation`: the host's libm (math.sin / math.cos, NOT numpy's, which may be a SIMD routine)
and the device's need not return the same bits, so rotation rows are compared with mpmath under a bar, not bit for bit.

EXACT VALUES.  The affine maps in `fractions.Fraction` (every input is a binary float, so the result is exact), atan2 / sin / cos in
mpmath at 200 bits.  `round_f32` gives the correctly rounded float32 of such a value and an "ambiguous" flag, set when the value lies
within the float64 evaluation's error of a float32 rounding midpoint -- there a correct float64 evaluation may round to either
neighbour.  The error bounds are
    affine maps  4 * 2^-53 * sum |terms|     (gather_ego: products, then three additions -- four rounded levels, each level's errors
                                              sum to at most 2^-53 of the terms' absolute sum.  to_origin has up to six levels; the
                                              products with the +-1 entries of Timg are exact and the six errors would all have to
                                              align to exceed this figure)
    atan2        4 * 2^-52 * |v|             (a libm atan2 within 2 ulp, doubled)
"""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

MP_BITS = 200
PI32 = np.float32(np.pi)
HALF_PI32 = np.float32(np.pi / 2)
SUB32 = np.float32(1e-40)                      # a float32 subnormal
TINY32 = np.uint32(1).view(np.float32)         # the smallest one
assert 0 < float(SUB32) < 2.0 ** -126 and float(TINY32) == 2.0 ** -149

# the pose of the issue's CPU case: translations (-8123.4567, 15234.789, -31.25), yaw 1.234, points around (6000, -14000, 30)
BIG_CENTRE = (6000.0, -14000.0, 30.0)


def big_pose():
    T = np.eye(4)
    c, s = math.cos(1.234), math.sin(1.234)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [-8123.4567, 15234.789, -31.25]
    return T


def translation_pose():
    T = np.eye(4)
    T[:3, 3] = [12.5, -3.25, 0.125]
    return T


def timg():
    """Rx(pi) @ Rz(pi/2) as scipy builds it (what RealisticProjection uploads): an INPUT of k_to_origin"""
    from scipy.spatial.transform import Rotation
    return np.ascontiguousarray(Rotation.from_euler('x', np.pi).as_matrix() @ Rotation.from_euler('z', np.pi / 2.).as_matrix())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def f32_steps(a, b):
    """distance in float32 steps (+0 and -0 are the same point of the line)"""
    def key(x):
        i = bits(np.asarray(x, np.float32)).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------------------------ restatements
def gather_ego(points, stride_cols, index, T):
    """k_gather_ego: ((T0 x + T1 y) + T2 z) + T3 in float64, rounded to float32.  points: float32, `stride_cols` floats per row;
    index: rows to take, or None"""
    p = np.asarray(points, np.float32).reshape(-1, stride_cols)
    if index is not None:
        p = p[np.asarray(index)]
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    T = np.asarray(T, np.float64)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def libm_sin_cos(a):
    a = np.asarray(a, np.float64).ravel()
    return np.array([math.sin(v) for v in a]), np.array([math.cos(v) for v in a])


def view_rotation(angle_f32, sin_cos=libm_sin_cos):
    """view_rotation of render.hip: rows {m00, m01, m10, m11, m22, angle} of scipy's Rotation.from_euler('z', -angle).as_matrix()"""
    ang = np.asarray(angle_f32, np.float32).ravel()
    a = -ang.astype(np.float64)
    s, w = sin_cos(a * 0.5)
    z2, w2, zw = s * s, w * w, s * w
    out = np.empty((len(ang), 6), np.float64)
    out[:, 0] = -z2 + w2
    out[:, 1] = 2.0 * (-zw)
    out[:, 2] = 2.0 * zw
    out[:, 3] = -z2 + w2
    out[:, 4] = z2 + w2
    out[:, 5] = ang.astype(np.float64)
    return out


def to_origin(ego, pt_cluster, med, rot, Timg):
    """k_to_origin: float32 subtraction of the median's x and y, then float64; rounded to float32"""
    ego, med = np.asarray(ego, np.float32), np.asarray(med, np.float32)
    c = np.asarray(pt_cluster)
    rot, Timg = np.asarray(rot, np.float64), np.asarray(Timg, np.float64)
    x = (ego[:, 0] - med[c, 0]).astype(np.float64)
    y = (ego[:, 1] - med[c, 1]).astype(np.float64)
    z = ego[:, 2].astype(np.float64)
    m = rot[c]
    q0 = m[:, 0] * x + m[:, 1] * y
    q1 = m[:, 2] * x + m[:, 3] * y
    q2 = m[:, 4] * z
    q0 = q0 - 1.0
    out = np.empty((len(ego), 3), np.float32)
    for r in range(3):
        out[:, r] = ((Timg[r, 0] * q2 + Timg[r, 1] * q1) + Timg[r, 2] * q0).astype(np.float32)
    return out


def point_clusters(seg_off):
    """per-point cluster id of packed clusters"""
    seg_off = np.asarray(seg_off, np.int64)
    return np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ exact values
def round_f32(v, err):
    """v, err: Fraction.  -> (float32 nearest to v, ties to even; True when v is within err of a rounding midpoint).  err == 0 says
    the evaluation is exact: nothing is ambiguous then, a tie included"""
    if v == 0:
        return np.float32(0.0), False
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)                     # spacing of float32 around v (subnormals: 2^-149)
    t = v / q
    r = np.float32(float(round(t) * q))                        # round(): ties to even; the product is a float32, so float() is exact
    assert np.isfinite(r)
    return r, err > 0 and abs(abs(t - math.floor(t)) - Fraction(1, 2)) * q <= err


def _fr(a):
    return [Fraction(float(v)) for v in np.asarray(a).ravel()]


def _is_f64(v):
    return Fraction(float(v)) == v                             # float(Fraction) is correctly rounded


def _affine(steps, terms):
    """steps: every exact intermediate of the float64 evaluation, terms: the products it sums.  When each intermediate is a float64
    the evaluation rounds nowhere (by induction over its operations) and its error is 0 -- an exact tie is then no ambiguity: both
    sides round it to even.  Otherwise the bound of the module docstring."""
    err = Fraction(0) if all(_is_f64(s) for s in steps) else 4 * Fraction(2) ** -53 * sum(abs(t) for t in terms)
    return round_f32(steps[-1], err)


def exact_gather_ego(points, stride_cols, index, T):
    """-> (float32 [n,3] correctly rounded T * [p, 1], bool [n,3] ambiguous)"""
    p = np.asarray(points, np.float32).reshape(-1, stride_cols)
    if index is not None:
        p = p[np.asarray(index)]
    Tf = _fr(np.asarray(T, np.float64)[:3])
    out, amb = np.empty((len(p), 3), np.float32), np.zeros((len(p), 3), bool)
    for i in range(len(p)):
        h = _fr(p[i, :3]) + [Fraction(1)]
        for r in range(3):
            terms = [Tf[r * 4 + k] * h[k] for k in range(4)]
            sums = [terms[0] + terms[1], terms[0] + terms[1] + terms[2], sum(terms)]
            out[i, r], amb[i, r] = _affine(terms + sums, terms)
    return out, amb


def exact_to_origin(ego, pt_cluster, med, rot, Timg):
    """The affine map of k_to_origin evaluated exactly on the float32 differences (the reference subtracts in float32 too:
    pointcloud_utils.py:399 works on a float32 array) -> (float32 [n,3], bool [n,3] ambiguous)"""
    ego, med = np.asarray(ego, np.float32), np.asarray(med, np.float32)
    c = np.asarray(pt_cluster)
    xs, ys = ego[:, 0] - med[c, 0], ego[:, 1] - med[c, 1]
    rot_f = [_fr(row[:5]) for row in np.asarray(rot, np.float64)]
    Tf = _fr(Timg)
    out, amb = np.empty((len(ego), 3), np.float32), np.zeros((len(ego), 3), bool)
    for i in range(len(ego)):
        x, y, z = Fraction(float(xs[i])), Fraction(float(ys[i])), Fraction(float(ego[i, 2]))
        m = rot_f[c[i]]
        w = [[m[4] * z], [m[2] * x, m[3] * y], [m[0] * x, m[1] * y, Fraction(-1)]]           # np.stack([z, y, x]) as lists of terms
        inner = [t for k in range(3) for t in w[k]] + [w[2][0] + w[2][1]] + [sum(wk) for wk in w]
        for r in range(3):
            terms = [Tf[r * 3 + k] * t for k in range(3) for t in w[k]]
            prods = [Tf[r * 3 + k] * sum(w[k]) for k in range(3)]
            out[i, r], amb[i, r] = _affine(inner + prods + [prods[0] + prods[1], sum(prods)], terms)
    return out, amb


def _mp_fraction(v):
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * Fraction(2) ** int(exp)
    return -f if sign else f


def exact_atan2(y, x):
    """float32 arrays without zeros -> (float32 correctly rounded atan2, bool ambiguous)"""
    y, x = np.asarray(y, np.float32).ravel(), np.asarray(x, np.float32).ravel()
    out, amb = np.empty(len(y), np.float32), np.zeros(len(y), bool)
    with mpmath.workprec(MP_BITS):
        for i in range(len(y)):
            assert y[i] != 0 and x[i] != 0
            v = _mp_fraction(mpmath.atan2(mpmath.mpf(float(y[i])), mpmath.mpf(float(x[i]))))
            out[i], amb[i] = round_f32(v, 4 * Fraction(2) ** -52 * abs(v))
    return out, amb


def rotation_error(rows):
    """[n,6] rotation rows -> [n,5] |entry - exact|, exact = (cos a, -sin a, sin a, cos a, 1) of a = -angle in mpmath.  The exact
    values are held as float64 pairs (hi + lo, good to ~2^-106), so the difference is formed without loss."""
    rows = np.asarray(rows, np.float64)
    hi, lo = _exact_rotation(np.ascontiguousarray(rows[:, 5].astype(np.float32)).tobytes())
    return np.abs((rows[:, :5] - hi) - lo)


@functools.lru_cache(maxsize=32)
def _exact_rotation(angle_bytes):
    ang = np.frombuffer(angle_bytes, np.float32)
    hi, lo = np.empty((len(ang), 5)), np.zeros((len(ang), 5))
    with mpmath.workprec(MP_BITS):
        for i, a in enumerate(ang):
            c, s = mpmath.cos_sin(-mpmath.mpf(float(a)))
            ch, sh = float(c), float(s)
            cl, sl = float(c - ch), float(s - sh)
            hi[i] = (ch, -sh, sh, ch, 1.0)
            lo[i] = (cl, -sl, sl, cl, 0.0)
    return hi, lo


# ------------------------------------------------------------------------------------------------------------------ inputs
def neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def edge_angles():
    """+-0, +-pi, +-pi/2 (float32) and their float32 neighbours, 1e-30, the smallest subnormal"""
    e = [np.float32(0.0), np.float32(-0.0)]
    for v in (PI32, -PI32, HALF_PI32, -HALF_PI32):
        e += neighbours(v)
    e += [np.float32(1e-30), TINY32, -TINY32, SUB32]
    return np.array(e, np.float32)


@functools.lru_cache(maxsize=1)
def rotation_angles():
    """the edge angles, then 100 000 seeded float32 angles in [-pi, pi]"""
    rng = np.random.default_rng(20)
    a = rng.uniform(-np.pi, np.pi, 100_000).astype(np.float32)
    a = np.clip(a, -PI32, PI32)
    out = np.concatenate([edge_angles(), a])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def host_rotation():
    """-> (rows of the libm restatement on rotation_angles(), E_host = their worst absolute error against mpmath)"""
    rows = view_rotation(rotation_angles())
    e_host = float(rotation_error(rows).max())
    rows.setflags(write=False)
    return rows, e_host


def rotation_bar(e_host):
    return max(8.0 * e_host, 2.0 ** -50)


def seeded_medians(n=4000, seed=21):
    """float32 medians at scales 1e-3 .. 80, all quadrants, no zeros"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, math.log10(80.0), (n, 1))
    m = (rng.normal(size=(n, 3)) * scale).astype(np.float32)
    m[m == 0] = np.float32(1.0)
    return m


def big_pose_points(n=3000, stride=5, seed=22):
    """float32 rows: xyz within +-40 m of BIG_CENTRE, NaN in the unused columns"""
    rng = np.random.default_rng(seed)
    p = np.full((n, stride), np.nan, np.float32)
    p[:, :3] = (np.array(BIG_CENTRE) + rng.uniform(-40, 40, (n, 3))).astype(np.float32)
    return p
