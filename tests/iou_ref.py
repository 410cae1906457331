"""Shared by tests/test_iou_host.py and tests/test_iou_device.py: the fixture of tests/golden/make_iou.py, the bar, the group layouts
and the seeded evaluation scenes.  TEST INFRASTRUCTURE ONLY: nothing here computes an expected IoU.

THE BAR.  Per pair, in every mode (mode 2 relative to the larger box's area):

    |kernel - reference|  <=  min( max(8 * E_host[family], 2^-50),  2^-50 + 2^-44 * R^2 / U )

First term: the issue's bar.  E_host is the host function's own worst error per family, measured by the generator and stored in the
fixture (family C stores the value of its origin-centred twins); 8 x is the margin tests/test_segment_edges.py gives the box kernel
over its float64 reference's own error; 2^-50 is the same 8 x on one rounding of a result <= 1.  The values in the committed fixture:
    A 5.551e-16   B 4.286e-10   C 4.286e-10   D 2.776e-16   E 3.343e-14
(B is large because iou3d_matrix treats edges within 1e-12 of parallel as parallel and takes vertices within 1e-9 as inside; that
says nothing about the kernel, hence the second term.)

Second term: from the kernel's arithmetic (csrc/iou_pair.inc), with eps = 2^-53, R = the sum of the two half-diagonals, U = the
larger box's area (<= the union's).  Every vertex of the clipped polygon lies within 2 R of B's centre and is the result of at most 12
roundings of values that size (centre difference 1, its rotation 3 + 2 for the sine / cosine, a corner 2 + 2 + 2), and a
crossing adds an interpolation along an edge no longer than 2 R: a vertex is off by <= 24 eps R.  Moving every vertex by d changes
the area by at most perimeter * d, the intersection's perimeter is at most a box's, <= 4 sqrt(2) * (its half-diagonal) < 5.7 R: the
area is off by < 137 eps R^2, the fan adds < 8 eps of the area, and IoU = I / (U' - I) has slope <= 2 / U' in I: < 290 eps R^2 / U,
rounded up to 512 eps = 2^-44.  For square-ish boxes that is ~1e-13 where the first term allows 3e-9; a kernel that forms
world-coordinate corners first is off by ~1e-13 .. 1e-12 at the centres of family C.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FAMILIES = 'ABCDE'
FLOOR = 2.0 ** -50


def fixture():
    g = np.load(os.path.join(GOLDEN, 'iou_golden.npz'))
    return {k: g[k] for k in g.files}


def areas(a, b):
    return np.maximum(a[:, 3] * a[:, 4], b[:, 3] * b[:, 4])


def bars(g):
    """-> [P] the bar of every fixture pair (module docstring)"""
    a, b = g['a'], g['b']
    issue = np.maximum(8.0 * g['e_host'][g['family']], FLOOR)
    reach = 0.5 * (np.hypot(a[:, 3], a[:, 4]) + np.hypot(b[:, 3], b[:, 4]))
    u = areas(a, b)
    own = FLOOR + 2.0 ** -44 * reach ** 2 / np.where(u > 0, u, 1.0)
    return np.where(u > 0, np.minimum(issue, own), issue)


def errors(g, got, mode):
    """|got - reference| of one mode, mode 2 relative to the larger box's area"""
    err = np.abs(np.asarray(got) - g['ref'][:, mode])
    if mode == 2:
        u = areas(g['a'], g['b'])
        err = err / np.where(u > 0, u, 1.0)
    return err


def check_against_bar(g, got_by_mode, label):
    """every family, every mode: inside the bar; exact zeros in family A; prints the share of the bar used (pytest -s)"""
    bar = bars(g)
    for mode in (0, 1, 2):
        got = np.asarray(got_by_mode[mode])
        assert got.shape == (len(bar),) and np.all(np.isfinite(got))
        err = errors(g, got, mode)
        for k, f in enumerate(FAMILIES):
            sel = g['family'] == k
            share = (err[sel] / bar[sel]).max()
            print(f'{label} mode {mode} family {f}: {int(sel.sum())} pairs, worst error {err[sel].max():.3e}, share of the bar {share:.3f}')
        worst = int(np.argmax(err / bar))
        assert np.all(err <= bar), (label, mode, FAMILIES[g['family'][worst]], worst, err[worst], bar[worst])
        zero = (g['family'] == 0) & (g['ref'][:, mode] == 0)
        assert zero.sum() >= 20 and np.all(got[zero] == 0.0), (label, mode, np.flatnonzero(zero & (got != 0)))


def one_group_per_pair(n):
    return np.arange(n + 1, dtype=np.int64)


def crowd(n, seed=0):
    """-> (a [n,7], b [n,7]) seeded boxes crowded into 16 m x 16 m around (20, -30): most cross pairs intersect.  Inputs only."""
    rng = np.random.default_rng(900 + seed)

    def draw():
        return np.c_[20 + rng.uniform(-8, 8, n), -30 + rng.uniform(-8, 8, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 6, n), rng.uniform(0.5, 3, n),
                     rng.uniform(1, 3, n), rng.uniform(-4, 4, n)]
    return draw(), draw()


# ---- seeded evaluation scenes --------------------------------------------------------------------------------------------------
SCENE_SEEDS = list(range(20))
SCENE_THRESHOLDS = (0.0, 0.5, 0.3, 0.4, 0.35)                # iou_thresholds[type], type 0 unused


def scene(seed):
    """3 frames, types 1, 2 and 4, up to 4 x 4 boxes per frame and type -> the nine positional arguments of detection_metrics but the config"""
    rng = np.random.default_rng(7000 + seed)
    pf, pb, pt, ps, gf, gb, gt, gl = [], [], [], [], [], [], [], []
    for f in range(3):
        for t in (1, 2, 4):
            ng, np_ = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            size = {1: (4.5, 2.0, 1.6), 2: (0.8, 0.7, 1.7), 4: (1.8, 0.7, 1.6)}[t]
            g = np.c_[rng.uniform(-30, 30, (ng, 2)), rng.uniform(-1, 1, ng), size * rng.uniform(0.8, 1.2, (ng, 3)), rng.uniform(-np.pi, np.pi, ng)]
            g = g.reshape(ng, 7)
            if ng and np_:
                src = rng.integers(0, ng, np_)
                p = g[src] + np.c_[rng.normal(0, 0.25, (np_, 2)) * size[0] / 2, rng.normal(0, 0.1, np_), rng.normal(0, 0.1, (np_, 3)),
                                   rng.normal(0, 0.2, np_)]
            else:
                p = np.c_[rng.uniform(-30, 30, (np_, 2)), rng.uniform(-1, 1, np_), size * rng.uniform(0.8, 1.2, (np_, 3)), rng.uniform(-np.pi, np.pi, np_)]
            p = p.reshape(np_, 7)
            pf += [f] * np_; pb.append(p); pt += [t] * np_; ps += list(np.round(rng.uniform(0.05, 0.99, np_), 3))
            gf += [f] * ng; gb.append(g); gt += [t] * ng; gl += list(rng.integers(1, 3, ng))
    return (np.array(pf, np.int64), np.concatenate(pb).reshape(-1, 7), np.array(pt, np.int64), np.array(ps, np.float64),
            np.array(gf, np.int64), np.concatenate(gb).reshape(-1, 7), np.array(gt, np.int64), np.array(gl, np.int8))


def scene_margins(seed, iou3d_matrix, cutoffs):
    """-> (smallest distance of a nonzero host IoU from its threshold, smallest lead of the best assignment over the second best over
    every (frame, type, distinct kept set)), the second by brute force over ALL injective partial assignments"""
    import itertools
    pf, pb, pt, ps, gf, gb, gt, _ = scene(seed)
    d_thr, lead = np.inf, np.inf
    for f in range(3):
        for t in (1, 2, 4):
            pi, gi = np.flatnonzero((pf == f) & (pt == t)), np.flatnonzero((gf == f) & (gt == t))
            if len(pi) == 0 or len(gi) == 0:
                continue
            iou = iou3d_matrix(pb[pi], gb[gi])
            thr = SCENE_THRESHOLDS[t]
            nz = iou[iou > 0]
            if len(nz):
                d_thr = min(d_thr, np.abs(nz - thr).min())
            w = np.where((iou >= thr) & (iou > 0), iou, 0.0)
            seen = set()
            for cut in cutoffs:
                keep = tuple(np.flatnonzero(ps[pi] >= cut))
                if keep in seen or not keep:
                    continue
                seen.add(keep)
                totals = {}
                for assign in itertools.product(range(-1, len(gi)), repeat=len(keep)):
                    used = [g for g in assign if g >= 0]
                    if len(used) != len(set(used)):
                        continue
                    pairs = frozenset((keep[k], g) for k, g in enumerate(assign) if g >= 0 and w[keep[k], g] > 0)
                    totals[pairs] = sum(w[p, g] for p, g in pairs)
                order = sorted(totals.values(), reverse=True)
                if len(order) > 1:
                    lead = min(lead, order[0] - order[1])
    return d_thr, lead
