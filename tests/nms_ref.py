"""Shared by tests/test_nms_host.py and tests/test_nms_device.py: the numpy greedy NMS the library is held to, the raw calls of the two
entry points (sentinel-filled outputs) and the cases.  TEST INFRASTRUCTURE ONLY.

THE REFERENCE.  `reference(case)` is a plain greedy pass in Python.  Its order is ONE np.lexsort on (row index, -score) (numpy sorts
NaN last); its pair values M[q, p] are
    rotated   vg_boxes_iou3d_host(a = boxes, b = boxes, VG_IOU_BEV), which tests/test_iou_host.py pins to 60-digit arithmetic;
    normal    the axis-aligned IoU in fractions.Fraction over the exact values of the inputs, compared exactly with the threshold.
Keep lists and counts must be EQUAL to the library's: there is no tolerance.  The normal-mode cases keep centres and extents on a
1/64 grid inside +-64 m (+ a translation by whole metres), where every step of the library's arithmetic but the final quotient is
exact and the quotient is never within rounding of a threshold except where it equals it.
"""
import ctypes
from fractions import Fraction

import numpy as np

import iou_ref
from vilgod_amd import iou, nms
from vilgod_amd._lib import lib

SENTINEL = -7
READ = [0, 1, 3, 4, 6]                 # the box values either mode reads


def case(boxes, scores, off, thresh, mode='rotated', pre_max=None, max_group=None):
    off = np.asarray(off, np.int64)
    return {'boxes': np.ascontiguousarray(boxes), 'scores': np.ascontiguousarray(scores), 'off': off, 'thresh': float(thresh), 'mode': mode,
            'pre_max': pre_max, 'max_group': int(np.diff(off).max()) if max_group is None and len(off) > 1 else int(max_group or 0)}


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def normal_fraction(a, b):
    """exact axis-aligned BEV IoU of a (later row) against b (kept row)"""
    ax, ay, adx, ady = (Fraction(float(a[k])) for k in (0, 1, 3, 4))
    bx, by, bdx, bdy = (Fraction(float(b[k])) for k in (0, 1, 3, 4))
    if adx <= 0 or ady <= 0 or bdx <= 0 or bdy <= 0:
        return Fraction(0)
    ix = min(ax + adx / 2, bx + bdx / 2) - max(ax - adx / 2, bx - bdx / 2)
    iy = min(ay + ady / 2, by + bdy / 2) - max(ay - ady / 2, by - bdy / 2)
    if ix <= 0 or iy <= 0:
        return Fraction(0)
    inter = ix * iy
    return inter / (adx * ady + bdx * bdy - inter)


def pair_values(boxes, mode):
    """-> value(q, p): the mode's value with a = row q, b = row p of `boxes` (one group)"""
    n = len(boxes)
    if mode == 'rotated':
        with np.errstate(all='ignore'):
            M = iou.iou_groups_host(boxes, [0, n], boxes, [0, n], iou.MODE_BEV)[0].reshape(n, n)
        return lambda q, p, t: bool(M[q, p] > t)
    F = [[Fraction(float(v)) if np.isfinite(v) else Fraction(0) for v in row[:5]] for row in boxes]      # (a non-finite row is never evaluated)
    E = [(x - dx / 2, x + dx / 2, y - dy / 2, y + dy / 2, dx * dy, dx > 0 and dy > 0) for x, y, _, dx, dy in F]      # exact edges and areas

    def over(q, p, t):                                           # the steps of normal_fraction on the prepared edges
        a, b = E[q], E[p]
        if not (a[5] and b[5]):
            return 0 > Fraction(t)
        ix, iy = min(a[1], b[1]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[2], b[2])
        if ix <= 0 or iy <= 0:
            return 0 > Fraction(t)
        inter = ix * iy
        return inter / (a[4] + b[4] - inter) > Fraction(t)
    return over


def reference(c, sentinel=SENTINEL):
    boxes, scores, off = c['boxes'], c['scores'], c['off']
    keep, counts = np.full(len(boxes), sentinel, np.int32), np.zeros(len(off) - 1, np.int32)
    for g in range(len(off) - 1):
        o0, n = int(off[g]), int(off[g + 1] - off[g])
        if n > c['max_group']:
            keep[o0:o0 + n], counts[g] = -1, -1
            continue
        b, s = boxes[o0:o0 + n, :7], scores[o0:o0 + n]
        order = np.lexsort((np.arange(n), -s))
        ok = ~np.isnan(s) & np.isfinite(b[:, READ].astype(np.float64)).all(1)
        over = pair_values(b, c['mode'])
        kept = []
        for q in order[:n if c['pre_max'] is None else min(n, c['pre_max'])]:
            if ok[q] and not any(over(q, p, c['thresh']) for p in kept):
                kept.append(q)
        keep[o0:o0 + n] = -1
        keep[o0:o0 + len(kept)] = o0 + np.array(kept, np.int64)
        counts[g] = len(kept)
    return keep, counts


# ---- the raw calls -------------------------------------------------------------------------------------------------------------------
def _dt(a):
    return nms._F32 if a.dtype == np.float32 else nms._F64


def _args(c):
    boxes = np.ascontiguousarray(c['boxes'][:, :7])
    assert boxes.dtype in (np.float32, np.float64) and c['scores'].dtype in (np.float32, np.float64)
    return boxes, c['scores'], np.ascontiguousarray(c['off'], np.int32), nms._MODES[c['mode']], c['pre_max'] or 0


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_raw(c, sentinel=SENTINEL):
    """vg_boxes_nms_host on sentinel-filled outputs -> (status, keep, counts)"""
    boxes, scores, off, mode, pre = _args(c)
    keep, counts = np.full(len(boxes), sentinel, np.int32), np.full(len(off) - 1, sentinel, np.int32)
    st = lib.vg_boxes_nms_host(_dt(boxes), _p(boxes), _dt(scores), _p(scores), _p(off), len(off) - 1, len(boxes), c['max_group'], mode,
                               c['thresh'], pre, _p(keep), _p(counts))
    return st, keep, counts


def device_raw(c, dev, sentinel=SENTINEL, work_fill=None):
    """vg_boxes_nms on sentinel-filled outputs (and a work buffer filled with `work_fill` bytes) -> (status, keep, counts)"""
    import torch
    from vilgod_amd._lib import ptr, stream_ptr
    boxes, scores, off, mode, pre = _args(c)
    d_boxes, d_scores, d_off = (torch.from_numpy(x).to(dev) for x in (boxes, scores, off))
    keep = torch.full((len(boxes),), sentinel, dtype=torch.int32, device=dev)
    counts = torch.full((len(off) - 1,), sentinel, dtype=torch.int32, device=dev)
    nbytes = int(lib.vg_boxes_nms_work_bytes(len(boxes), c['max_group'], len(off) - 1))
    work = torch.full((max(nbytes, 8),), 0 if work_fill is None else work_fill, dtype=torch.uint8, device=dev)
    st = lib.vg_boxes_nms(_dt(boxes), ptr(d_boxes), _dt(scores), ptr(d_scores), ptr(d_off), len(off) - 1, len(boxes), c['max_group'], mode,
                          c['thresh'], pre, ptr(work), ptr(keep), ptr(counts), stream_ptr(torch.cuda.current_stream(dev)))
    return st, keep.cpu().numpy(), counts.cpu().numpy()


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def crowd(n, seed, dtype=np.float64):
    return iou_ref.crowd(n, seed)[0].astype(dtype)


def crowd_scores(n, seed, dtype=np.float64):
    return np.random.default_rng(4100 + seed).uniform(0.05, 0.99, n).astype(dtype)


def grid_crowd(n, seed, span=8.0):
    """centres and extents on a 1/64 grid, crowded into 2 span x 2 span; headings arbitrary"""
    rng = np.random.default_rng(5200 + seed)
    g = lambda lo, hi, k: rng.integers(int(lo * 64), int(hi * 64) + 1, k) / 64.0
    return np.c_[g(-span, span, n), g(-span, span, n), rng.uniform(-1, 1, n), g(0.5, 6, n), g(0.5, 3, n), rng.uniform(1, 3, n), rng.uniform(-4, 4, n)]


def far_boxes(n, seed=0):
    """n boxes that touch nothing: 10 m apart on a line far from the origin"""
    rng = np.random.default_rng(6300 + seed)
    return np.c_[500.0 + 10.0 * np.arange(n), np.full(n, 300.0), np.zeros(n), rng.uniform(1, 4, n), rng.uniform(1, 2, n), np.ones(n), rng.uniform(-3, 3, n)]


CHAIN = np.array([[0.0, 0, 0, 2, 1, 1, 0], [0.5, 0, 0, 2, 1, 1, 0], [1.0, 0, 0, 2, 1, 1, 0]])      # A/B and B/C 0.6, A/C 1/3
EDGE = np.array([[0.0, 0, 0, 2, 1, 1, 0], [0.5, 0, 0, 1, 1, 1, 0]])                                # the 1 x 1 inside the 2 x 1: 0.5


def seam_case(mode='rotated', dtype=np.float64, seed=0, thresh=0.3):
    """group sizes 0, 1, 2, 63, 64, 65, 127, 128, 129 and 1000, 300 groups of 1, empty groups in the middle, slack at both ends"""
    sizes = [0, 1, 2, 63, 64, 0, 0, 65, 127, 128, 129, 0, 1000] + [1] * 300 + [0, 3]
    off = 5 + np.cumsum([0] + sizes)
    n = int(off[-1]) + 4
    rng = np.random.default_rng(7400 + seed)
    boxes = np.zeros((n, 7))
    for g, s in enumerate(sizes):                              # each group is its own crowd, dense enough that most rows meet several
        b = grid_crowd(s, 100 * seed + g, span=min(8.0, 1.0 + s / 40.0))
        boxes[off[g]:off[g] + s] = b
    if mode == 'rotated':
        boxes[:, READ] += rng.uniform(-0.01, 0.01, (n, 5))    # off the grid
    return case(boxes.astype(dtype), rng.uniform(0, 1, n).astype(dtype), off, thresh, mode)


def chain_cases(mode='rotated'):
    out = {}
    A, B, C = CHAIN
    out['chain'] = case(CHAIN, np.array([0.9, 0.8, 0.7]), [0, 3], 0.5, mode)
    out['chain_b_first'] = case(CHAIN, np.array([0.8, 0.9, 0.7]), [0, 3], 0.5, mode)
    far = far_boxes(63)
    out['chain_seam'] = case(np.r_[far, CHAIN], np.r_[np.linspace(2, 3, 63), [0.9, 0.8, 0.7]], [0, 66], 0.5, mode)       # ranks 63, 64, 65
    far = far_boxes(200)
    boxes = np.r_[A[None], far[:100], B[None], far[100:], C[None]]
    scores = np.r_[[0.9], np.linspace(0.85, 0.81, 100), [0.8], np.linspace(0.79, 0.71, 100), [0.7]]
    out['chain_apart'] = case(boxes, scores, [0, 203], 0.5, mode)
    order = np.random.default_rng(1).permutation(203)
    out['chain_apart_shuffled'] = case(boxes[order], scores[order], [0, 203], 0.5, mode)
    return out


def order_cases(mode='rotated'):
    out = {}
    b = grid_crowd(150, 11, span=4.0)
    out['equal_scores'] = case(b, np.full(150, 0.5), [0, 150], 0.3, mode)
    out['ascending'] = case(b, np.linspace(0.1, 0.9, 150), [0, 150], 0.3, mode)
    out['descending'] = case(b, np.linspace(0.9, 0.1, 150), [0, 150], 0.3, mode)
    out['shuffled'] = case(b, np.random.default_rng(2).permutation(np.linspace(0.1, 0.9, 150)), [0, 150], 0.3, mode)
    s = np.full(150, 0.7, np.float32)
    s[::3] = np.nextafter(np.float32(0.7), np.float32(1))
    s[1::3] = np.nextafter(np.float32(0.7), np.float32(0))
    out['last_bit_f32'] = case(b, s, [0, 150], 0.3, mode)
    z = np.where(np.arange(150) % 2 == 0, 0.0, -0.0)          # +0.0 and -0.0 are one score
    out['signed_zero'] = case(b, z, [0, 150], 0.3, mode)
    return out


def padding_case(mode='rotated', dtype=np.float64):
    """NaN scores, +-inf scores, rows with NaN / +-inf coordinates -- one of them a duplicate of the best box with a NaN score, one a
    duplicate of it with the highest score and a NaN heading"""
    b = grid_crowd(140, 21, span=4.0)
    s = np.random.default_rng(3).uniform(0.1, 0.9, 140)
    best = 40
    s[best] = 0.94
    b[11, :2] = 60.0                                         # (the +inf score below stands apart: row `best` leads the crowd)
    b[5], s[5] = b[best], np.nan
    b[6], s[6] = b[best], 0.95
    b[6, 6] = np.nan
    s[[10, 70]] = np.nan
    s[11], s[12] = np.inf, -np.inf
    b[20, 0], b[21, 1], b[22, 3], b[23, 4], b[24, 6] = np.nan, np.inf, -np.inf, np.nan, np.inf
    s[20] = 0.99
    return case(b.astype(dtype), s.astype(dtype), [0, 140], 0.3, mode), best


def threshold_cases(mode='rotated'):
    out = {}
    s2 = np.array([0.9, 0.8])
    out['edge_at'] = case(EDGE, s2, [0, 2], 0.5, mode)
    out['edge_below'] = case(EDGE, s2, [0, 2], np.nextafter(0.5, 0), mode)
    out['edge_at_swapped'] = case(EDGE, s2[::-1].copy(), [0, 2], 0.5, mode)
    out['edge_below_swapped'] = case(EDGE, s2[::-1].copy(), [0, 2], np.nextafter(0.5, 0), mode)
    b = grid_crowd(40, 31, span=3.0)
    b[:, 6] = 0.0
    dup = np.r_[b, b]
    s = np.r_[np.linspace(0.9, 0.5, 40), np.linspace(0.45, 0.1, 40)]
    out['duplicates_at_one'] = case(dup, s, [0, 80], 1.0, mode)
    out['minus_one'] = case(np.r_[b, far_boxes(30)], np.random.default_rng(4).uniform(0, 1, 70), [0, 30, 30, 70], -1.0, mode)
    touch = np.array([[0.0, 0, 0, 2, 1, 1, 0], [2.0, 0, 0, 2, 1, 1, 0], [0.0, 1.0, 0, 2, 1, 1, 0], [2.0, 1.0, 0, 2, 1, 1, 0]])
    out['touching_at_zero'] = case(touch, np.array([0.4, 0.3, 0.2, 0.1]), [0, 4], 0.0, mode)
    return out


def pre_max_cases(mode='rotated'):
    b = grid_crowd(130, 41, span=4.0)
    s = np.random.default_rng(5).uniform(0, 1, 130)
    s[7] = np.nan
    return {f'pre_max_{k}': case(np.r_[b, b[:20]], np.r_[s, s[:20]], [0, 130, 150], 0.3, mode, pre_max=k) for k in (1, 64, 65, 130, 5000)}


def crowd_case(n, seed, thresh, dtype, mode='rotated'):
    return case(crowd(n, seed, dtype), crowd_scores(n, seed), [0, n], thresh, mode)


def ordered_pairs_case(g, thresh, mode='normal'):
    """one 2-row group per ordered pair (q, p), q != p, of the boxes g: p leads, so group k's count is 1 iff v(q, p) > thresh
    -> (case, q, p)"""
    n = len(g)
    q, p = (x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
    q, p = q[q != p], p[q != p]
    boxes = np.empty((2 * len(q), 7))
    boxes[0::2], boxes[1::2] = g[p], g[q]
    return case(boxes, np.tile([1.0, 0.0], len(q)), 2 * np.arange(len(q) + 1), thresh, mode), q, p


def small_group_case(mode='rotated'):
    """max_group smaller than a real group: that group comes back as -1, the others right"""
    b = np.r_[grid_crowd(50, 51, span=3.0), grid_crowd(90, 52, span=3.0), grid_crowd(40, 53, span=3.0)]
    return case(b, np.random.default_rng(6).uniform(0, 1, 180), [0, 50, 140, 180], 0.3, mode, max_group=64)


def all_cases():
    """-> {name: case}: every case of tests/test_nms_host.py, for the device test to run through vg_boxes_nms"""
    out = {}
    for mode in ('rotated', 'normal'):
        tag = mode[0] + ':'
        out[tag + 'seams_f64'] = seam_case(mode, np.float64)
        out[tag + 'seams_f32'] = seam_case(mode, np.float32, seed=1)
        for fam in (chain_cases, order_cases, threshold_cases, pre_max_cases):
            out.update({tag + k: v for k, v in fam(mode).items()})
        out[tag + 'padding_f64'] = padding_case(mode, np.float64)[0]
        out[tag + 'padding_f32'] = padding_case(mode, np.float32)[0]
        out[tag + 'small_max_group'] = small_group_case(mode)
    for n in (129, 512):
        for seed in (0, 1, 2):
            for t in (0.1, 0.5, 0.7):
                for dt in (np.float32, np.float64):
                    out[f'crowd_{n}_{seed}_{t}_{np.dtype(dt).name}'] = crowd_case(n, seed, t, dt)
    g = grid_crowd(300, 61)
    for t in (0.1, 0.25, 0.5, 0.7):
        out[f'n:grid_{t}'] = case(g, crowd_scores(300, 9), [0, 300], t, 'normal')
    out['n:ordered_pairs'] = ordered_pairs_case(g, 0.25)[0]
    out['r:ordered_pairs'] = ordered_pairs_case(crowd(120, 4), 0.1, 'rotated')[0]
    return out
