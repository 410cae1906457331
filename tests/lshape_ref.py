"""Numpy restatement of the two L-shape box fits of fit_bounding_boxes_simple (closeness_rectangle and variance_rectangle,
pointcloud_utils.py:170-288 of the reference), for the tests of csrc/lshape.hip.

The fit sweeps the heading a over angles(delta).  At each a the cluster's xy points are projected on the two axes of a; every
point has a distance Dx to the nearer end of the x extent and Dy to the nearer end of the y extent.
  closeness: criterion = sum 1 / max(min(Dx, Dy), delta_zero)   (points hugging an edge score high)
  variance:  criterion = -var(Dx of the points nearer an x end) - var(Dy of the points nearer a y end)   (ddof 0; empty side: 0)
The fit is the FIRST a of the largest criterion.  At that a the rectangle is turned by a right angle when its x side is the shorter.

Dtypes: closeness projects in float32 (its axes are float32), variance in float64.  Closeness accumulates 1 / beta in float64 with
numba=True -- how the reference runs, since numba types `np.maximum(float32 array, 1e-2)` as float64 -- and in float32 with
numba=False: the same body under plain numpy, which is what tests/golden/make_lshape.py recorded (numba is not installed there).
Projections are rounded as numpy's dot rounds them (BLAS gemm: fma(y, s, x * c)); `_proj` reproduces that with one float64 sum,
exact for float32 operands.
"""
import numpy as np

PI2 = np.pi / 2
DEFAULTS = {'closeness_rectangle': {'delta': 2, 'delta_zero': 1e-2}, 'variance_rectangle': {'delta': 0.1}}


def angles(delta):
    return np.arange(0, 90 + delta, delta) / 180. * np.pi


def _axes(a, dtype):
    """the heading's two axes as rows, [[c, s], [-s, c]] in `dtype`"""
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, s], [-s, c]], dtype=dtype)


def _proj(xy, m):
    """xy @ m with each element rounded as gemm does: the first product rounded, the second added by one fused multiply-add"""
    if m.dtype == np.float32:
        x, y = xy[:, :1].astype(np.float32), xy[:, 1:2].astype(np.float32)
        first = (x * m[0]).astype(np.float64)
        return (first + y.astype(np.float64) * m[1].astype(np.float64)).astype(np.float32)
    return np.dot(np.asarray(xy, np.float64), m)


def _near(p):
    lo, hi = p.min(axis=0), p.max(axis=0)
    return np.minimum(p - lo, hi - p)


def criteria(xy, name, numba=True, **args):
    """[A] criterion of every angle."""
    args = dict(DEFAULTS[name], **args)
    xy = np.asarray(xy, np.float32)
    out = []
    for a in angles(args['delta']):
        if name == 'closeness_rectangle':
            d = _near(np.dot(xy, _axes(a, np.float32).T))
            beta = np.minimum(d[:, 0], d[:, 1])
            if numba:
                out.append(np.sum(1.0 / np.maximum(beta.astype(np.float64), args['delta_zero'])))
            else:
                out.append((1 / np.maximum(beta, args['delta_zero'])).sum())
        else:
            d = _near(np.dot(xy, _axes(a, np.float64).T))
            ex, ey = d[d[:, 0] < d[:, 1], 0], d[d[:, 1] < d[:, 0], 1]
            v = 0
            if len(ex):
                v += -np.var(ex)
            if len(ey):
                v += -np.var(ey)
            out.append(v)
    return np.array(out, dtype=np.float64)


def criteria_fast(xy, name, **args):
    """criteria(numba=True) with all angles at once (for thousands of clusters); the sums run in another order."""
    args = dict(DEFAULTS[name], **args)
    a = angles(args['delta'])
    dt = np.float32 if name == 'closeness_rectangle' else np.float64
    c, s = np.cos(a).astype(dt), np.sin(a).astype(dt)
    xy = np.asarray(xy, np.float32)
    u = _near(_proj(xy, np.stack([c, s])))
    v = _near(_proj(xy, np.stack([-s, c])))
    if name == 'closeness_rectangle':
        beta = np.minimum(u, v).astype(np.float64)
        return (1.0 / np.maximum(beta, args['delta_zero'])).sum(axis=0)
    out = np.zeros(len(a))
    for d, o in ((u, v), (v, u)):
        m = d < o
        n = m.sum(axis=0)
        mean = np.where(m, d, 0).sum(axis=0) / np.maximum(n, 1)
        var = np.where(m, (d - mean) ** 2, 0).sum(axis=0) / np.maximum(n, 1)
        out -= np.where(n > 0, var, 0)
    return out


def fit(xy, name, crit=None, numba=True, **args):
    """-> (chosen index, corners [4,2] in the fit's dtype, rz before the l/w swap, criterion vector)."""
    args = dict(DEFAULTS[name], **args)
    if crit is None:
        crit = criteria(xy, name, numba=numba, **args)
    k = int(np.argmax(crit))                     # the first maximum (the reference's strict `>` from -inf)
    dt = np.float32 if name == 'closeness_rectangle' else np.float64
    xy = np.asarray(xy, np.float32)
    a = angles(args['delta'])[k]
    m = _axes(a, dt)
    p = np.dot(xy, m.T)
    if p[:, 0].max() - p[:, 0].min() < p[:, 1].max() - p[:, 1].min():
        a = a + PI2
        m = _axes(a, dt)
        p = np.dot(xy, m.T)
    x0, x1, y0, y1 = p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()
    corners = np.dot(np.array([[x1, y0], [x0, y0], [x0, y1], [x1, y1]], dtype=dt), m)
    return k, corners, a, crit


def box(corners, rz, z):
    """zero_shot_detector.py:452-461 with this numpy's promotion (float32 corners keep l, w and the centre float32; z float32)."""
    l = np.linalg.norm(corners[0] - corners[1])
    w = np.linalg.norm(corners[0] - corners[-1])
    c = (corners[0] + corners[2]) / 2
    if w > l:
        l, w = w, l
        rz += PI2
    z = np.asarray(z, np.float32)
    h = z.max() - z.min()
    return np.array([c[0], c[1], z.min() + h / 2, l, w, h + 0.3, rz])


def near_tie(crit, i, j, rtol):
    """criteria at indices i and j within rtol of each other (relative to the larger magnitude)"""
    a, b = crit[i], crit[j]
    return abs(a - b) <= rtol * max(abs(a), abs(b), 1e-300)
