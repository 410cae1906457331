"""Shared helpers of the ground-segmentation tests (tests/test_ground.py, tests/test_ground_edges.py): the kernel == oracle
equality that every GPU test asserts, and generated scenes that drive csrc/ground.hip into the branches its ordinary inputs
never reach (TGR, R-VPF, full and wrapped threshold stores, patch-size thresholds, binning edges).

Every scene is built patch by patch from the concentric-zone geometry, so which patch a point falls into is known by
construction; points keep a margin to ring and sector boundaries unless the scene is about those boundaries.
All scenes are in the sensor frame (z_offset = 0) and meant for min_range = 1.5.
"""
import numpy as np

from oracle import patchworkpp as opw

GROUND_Z = -1.72
MIN_RANGE = 1.5


# ------------------------------------------------------------------------------------------- the equality
def oracle_for(min_range=MIN_RANGE, tweak=None):
    p = opw.Parameters()
    p.min_range = min_range
    if tweak:
        tweak(p)
    return opw.patchworkpp(p)


def same_frame(oracle, gpu, pts, z_offset, k=0, num_min_pts=10):
    """One frame through both: the ground index set, the adaptive state and the patch records must be equal."""
    from vilgod_amd import patchworkpp as gpw
    want = np.sort(opw.mask_ground_points(pts, oracle, z_offset))
    got = np.sort(gpw.mask_ground_points_patchwork_pp(pts, gpu, z_offset))
    assert np.array_equal(want, got), (k, len(want), len(got), len(np.setxor1d(want, got)))
    so, sg = oracle.state(), gpu.state()
    assert so['sensor_height'] == sg['sensor_height'], k
    assert np.array_equal(so['elevation_thr'], sg['elevation_thr']) and np.array_equal(so['flatness_thr'], sg['flatness_thr'])
    assert np.array_equal(so['n_elevation'], sg['n_elevation']) and np.array_equal(so['n_flatness'], sg['n_flatness'])
    io, ig = oracle.patch_info(), gpu.patch_info()
    assert np.array_equal(io[:, :2], ig[:, :2]), k                       # sizes and inlier counts per patch
    live = io[:, 0] >= min(10, num_min_pts)
    assert np.array_equal(io[live, 2:11], ig[live, 2:11], equal_nan=True), k   # normals, means, singular values: bit exact


def _same_sequence(frames, z_offset, cuda, min_range=1.5, tweak=None, return_oracle=False):
    from vilgod_amd import patchworkpp as gpw
    po, pg = opw.Parameters(), gpw.Parameters()
    for p in (po, pg):
        p.min_range = min_range
        if tweak:
            tweak(p)
    oracle = opw.patchworkpp(po)
    gpu = gpw.patchworkpp(pg, max_points=max(len(f) for f in frames) + 1, device=cuda)
    for k, pts in enumerate(frames):
        same_frame(oracle, gpu, pts, z_offset, k, po.num_min_pts)
    return (gpu, oracle) if return_oracle else gpu


def oracle_masks(frames, tweak=None, min_range=MIN_RANGE):
    """-> (boolean masks, counters, states) per frame of a fresh oracle."""
    o = oracle_for(min_range, tweak)
    masks, counts, states = [], [], []
    for f in frames:
        m = np.zeros(len(f), bool)
        m[opw.mask_ground_points(f, o, 0.0)] = True
        masks.append(m)
        counts.append(o.counts())
        states.append(o.state())
    return masks, counts, states


# ------------------------------------------------------------------------------------------- geometry
class Geometry:
    """The concentric zone model (patchworkpp.h:116-131): ring bounds and sector counts per concentric index."""

    def __init__(self, min_range=MIN_RANGE, max_range=80.0, sectors=(16, 32, 54, 32), rings=(2, 4, 4, 4)):
        z = [min_range, (7 * min_range + max_range) / 8.0, (3 * min_range + max_range) / 4.0, (min_range + max_range) / 2.0, max_range]
        self.zone_bounds = z
        self.sectors, self.rings = tuple(sectors), tuple(rings)
        self.ring_lo, self.ring_hi, self.ring_sectors, self.ring_base = [], [], [], []
        base = 0
        for k in range(4):
            w = (z[k + 1] - z[k]) / rings[k]
            for r in range(rings[k]):
                self.ring_lo.append(z[k] + r * w)
                self.ring_hi.append(z[k] + (r + 1) * w)
                self.ring_sectors.append(sectors[k])
                self.ring_base.append(base)
                base += sectors[k]
        self.n_patches = base
        self.n_rings = len(self.ring_lo)

    def pid(self, cidx, sector):
        return self.ring_base[cidx] + sector


DEFAULT = Geometry()


def patch_points(rng, n, cidx, sector, geom=DEFAULT, z0=GROUND_Z, noise=0.02, th_frac=(0.05, 0.95), r_frac=(0.05, 0.95),
                 intensity=(0.3, 1.0)):
    """n points inside patch (cidx, sector): r and theta uniform inside the given fractions of the patch, z = z0 + N(0, noise)."""
    lo, hi = geom.ring_lo[cidx], geom.ring_hi[cidx]
    ss = 2 * np.pi / geom.ring_sectors[cidx]
    r = lo + (hi - lo) * rng.uniform(r_frac[0], r_frac[1], n)
    th = ss * (sector + rng.uniform(th_frac[0], th_frac[1], n))
    z = z0 + noise * rng.normal(size=n)
    return np.stack([r * np.cos(th), r * np.sin(th), z, rng.uniform(intensity[0], intensity[1], n)], 1).astype(np.float32)


def ground(rng, per_patch, rings, geom=DEFAULT, z0=GROUND_Z, noise=(0.01, 0.026), skip=(), slope=0.0):
    """Flat ground over the given concentric rings: `per_patch` points in every patch, one noise level per patch drawn from
    `noise`; patches in `skip` ((cidx, sector) pairs) stay empty."""
    out = []
    for c in rings:
        for s in range(geom.ring_sectors[c]):
            if (c, s) in skip:
                continue
            n = per_patch[c] if isinstance(per_patch, (list, tuple, dict)) else per_patch
            out.append(patch_points(rng, n, c, s, geom, z0 + slope * geom.ring_lo[c], rng.uniform(*noise)))
    return np.concatenate(out)


NEAR = (0, 1, 2, 3)
# 60 000 points over r < 21.1 (concentric rings 0..5, what the issue measured its TGR scene on)
_TGR_PER_PATCH = {0: 900, 1: 900, 2: 230, 3: 230, 4: 230, 5: 230}


# ------------------------------------------------------------------------------------------- TGR
def tgr_scene(seed=0):
    """Three frames.  Frame 0 is flat ground (per-patch noise 0.01 ... 0.026), which sets the elevation and flatness thresholds.
    Frames 1 and 2 raise some patches by 0.3 m, above their ring's elevation threshold, with a noise that puts their flatness
    above the flatness threshold: TGR candidates.  What decides each candidate:
      noise 0.0245, few points           flatness below mean + 1.5 sigma of the ring: reverted by the sigmoid
      noise 0.05, few points             rejected by the sigmoid
      noise 0.05, > 1500 inliers         the sigmoid says no, `n_ground > 1500 && flatness < th_dist^2` reverts
      noise 0.0245, a radial strip       sv[0] / sv[1] > 8: rejected by line_variable although the sigmoid says yes
    Frame 1 has them in ring 0 and in ring 2 (zone 1, 32 sectors): ring 2's statistics still hold ring 1's values.  Frame 2 has
    them in rings 1, 2 and 3, each right after a ring that had candidates."""
    rng = np.random.default_rng(seed)
    rings = tuple(_TGR_PER_PATCH)

    def frame(special):
        parts = [ground(rng, _TGR_PER_PATCH, rings, skip=set(special))]
        for (c, s), kind in special.items():
            n = _TGR_PER_PATCH[c]
            if kind == 'mild':
                parts.append(patch_points(rng, n, c, s, z0=GROUND_Z + 0.3, noise=0.0245))
            elif kind == 'rough':
                parts.append(patch_points(rng, n, c, s, z0=GROUND_Z + 0.3, noise=0.05))
            elif kind == 'rough_big':
                parts.append(patch_points(rng, 2600, c, s, z0=GROUND_Z + 0.3, noise=0.05))
            elif kind == 'strip':
                parts.append(patch_points(rng, n, c, s, z0=GROUND_Z + 0.3, noise=0.0245, th_frac=(0.4, 0.6) if c < 2 else (0.45, 0.55)))
            elif kind == 'above':                  # a flat patch above the sensor: upright, but its heading points inside
                parts.append(patch_points(rng, n, c, s, z0=1.0, noise=0.02))
        f = np.concatenate(parts)
        return f[rng.permutation(len(f))]

    f0 = frame({})
    f1 = frame({(0, 3): 'mild', (0, 7): 'rough', (0, 9): 'rough_big', (0, 12): 'strip',
                (2, 5): 'mild', (2, 6): 'rough', (2, 20): 'rough_big', (2, 30): 'strip'})
    f2 = frame({(1, 2): 'mild', (1, 10): 'rough_big', (2, 9): 'rough', (2, 17): 'mild', (3, 0): 'strip', (3, 31): 'mild', (3, 15): 'rough_big', (1, 14): 'above'})
    return [f0, f1, f2]


def tgr_off(p):
    p.enable_TGR = 0


# ------------------------------------------------------------------------------------------- R-VPF
def wall(rng, n=3000, x=4.0, y=(0.3, 1.2), z=(-2.3, 0.5)):
    return np.stack([np.full(n, x) + rng.normal(0, 0.005, n), rng.uniform(y[0], y[1], n), rng.uniform(z[0], z[1], n),
                     rng.uniform(0.3, 1.0, n)], 1).astype(np.float32)


def rvpf_scene(n_patch, seed=1, wall_x=4.0, with_wall_only_patch=False):
    """One frame: ground over the near rings, `n_patch` ground points in the patch (ring 0, sector 0) and a 3000-point wall at
    x = 4 inside that patch that reaches from z = -2.3, below the ground, to 0.5.  The lowest points of the patch are wall
    points: R-VPF fits a vertical plane to them and removes the wall's foot before the ground fit; without it the seeds are wall
    points.  The patch holds n_patch + 3000 points: 4000 stays in LDS, 6000 and 18000 take the two big-patch paths that keep
    the alive flags in the inlier array."""
    rng = np.random.default_rng(seed)
    c = 0 if wall_x < 11 else 2
    parts = [ground(rng, 300, NEAR, skip={(c, 0)}), patch_points(rng, n_patch, c, 0), wall(rng, x=wall_x)]
    if with_wall_only_patch:                   # a patch that is nothing but wall: R-VPF removes it until nothing is left to fit
        w = wall(rng, n=800, x=3.0, y=(-0.4, -0.2), z=(-2.3, 0.5))
        parts += [w]
    f = np.concatenate(parts)
    return [f[rng.permutation(len(f))]]


def rvpf_off(p):
    p.enable_RVPF = 0


# ------------------------------------------------------------------------------------------- stores
def store_frames(n_frames, geom=DEFAULT, per_patch=40, seed=2, cycle=8):
    """Small frames confined to the four near rings (r < 16.2): `cycle` base frames repeat, z moves a little from frame to
    frame (a slow tilt of the whole scene plus a step), so the thresholds keep moving while the stores fill, evict and wrap."""
    rng = np.random.default_rng(seed)
    base = [ground(rng, per_patch, NEAR, geom, noise=(0.01, 0.03)) for _ in range(cycle)]
    frames = []
    for k in range(n_frames):
        f = base[k % cycle].copy()
        f[:, 2] += np.float32(0.004 * np.sin(0.37 * k) + 0.0007 * (k % 5))
        frames.append(f)
    return frames


def sectors64(p):
    for k in range(4):
        p.num_sectors_each_zone[k] = 64


GEOM64 = Geometry(sectors=(64, 64, 64, 64))


# ------------------------------------------------------------------------------------------- patch sizes
PATCH_SIZES = (9, 10, 11, 63, 64, 65, 255, 256, 257, 2049, 4095, 4096, 4097, 8193, 16383, 16384, 16385)


def patch_size_slots():
    """size -> (cidx, sector).  Ring 0 has 16 sectors and there are 17 sizes: 9, 10 and 11 sit in ring 1 (zone 0 as well),
    the other fourteen in ring 0 sectors 0..13; sectors 14 and 15 of ring 0 hold ordinary ground."""
    slots = {}
    for i, n in enumerate(PATCH_SIZES[:3]):
        slots[n] = (1, 2 + 3 * i)
    for i, n in enumerate(PATCH_SIZES[3:]):
        slots[n] = (0, i)
    return slots


def patch_size_scene(seed=3):
    """Two frames with the same points in two orders.  z is rounded to centimetres (many exact ties), clipped below at -1.80, and
    25 points of every patch that has them sit exactly at -1.80: the tie group straddles the num_lpr = 20 seed cut."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, (c, s) in patch_size_slots().items():
        p = patch_points(rng, n, c, s, noise=0.03)
        z = np.maximum(np.round(p[:, 2].astype(np.float64), 2), -1.80)
        z[rng.permutation(n)[:25]] = -1.80
        p[:, 2] = z.astype(np.float32)
        parts.append(p)
    parts += [patch_points(rng, 500, 0, 14), patch_points(rng, 500, 0, 15)]
    f = np.concatenate(parts)
    return [f[rng.permutation(len(f))], f[rng.permutation(len(f))]]


# ------------------------------------------------------------------------------------------- binning edges
def binning_edge_points():
    """Points whose bin is decided by an exact comparison: on the four half-axes (atan2 is exact there; y = -0.0 included) at
    r = min_range, max_range and the three zone boundaries (exact at min_range = 1.5) and at the next float above the two range
    limits; NaN / inf coordinates; z == FLT_MIN."""
    f32 = np.float32
    radii = [f32(1.5), np.nextafter(f32(1.5), f32(2)), f32(80.0), np.nextafter(f32(80.0), f32(81)), f32(11.3125), f32(21.125), f32(40.75),
             f32(5.0), f32(30.0)]
    pts = []
    for r in radii:
        for x, y in ((r, f32(0.0)), (r, f32(-0.0)), (f32(0.0), r), (f32(-0.0), r), (-r, f32(0.0)), (-r, f32(-0.0)), (f32(0.0), -r), (f32(-0.0), -r)):
            pts.append([x, y, GROUND_Z, 0.5])
    nan, inf = np.nan, np.inf
    pts += [[nan, 1.0, GROUND_Z, 0.5], [3.0, nan, GROUND_Z, 0.5], [nan, nan, nan, nan], [inf, 0.0, GROUND_Z, 0.5],
            [0.0, -inf, GROUND_Z, 0.5], [-inf, inf, GROUND_Z, 0.5], [inf, nan, -inf, 0.1]]
    pts += [[5.0, 1.0, np.finfo(np.float32).tiny, 0.5], [-7.0, 2.0, np.finfo(np.float32).tiny, 0.5]]
    return np.array(pts, dtype=np.float32)


def binning_scene(seed=4):
    """Ordinary ground over all fourteen rings (every patch live) plus the edge points, in two orders."""
    rng = np.random.default_rng(seed)
    g = ground(rng, 24, range(DEFAULT.n_rings), noise=(0.01, 0.02))
    e = binning_edge_points()
    return [np.concatenate([g, e]), np.concatenate([e, g[::-1]])], len(g), len(e)


# ------------------------------------------------------------------------------------------- one stored value
def single_value_scene(seed=5):
    """Frame 0: points in one ring-0 patch only, so every store of ring 0 receives exactly one value (mean and deviation stay 0,
    the elevation threshold becomes 0 and the sensor height -0).  Frame 1: ordinary ground over the near rings."""
    rng = np.random.default_rng(seed)
    return [patch_points(rng, 400, 0, 5), ground(rng, 40, NEAR)]


# ------------------------------------------------------------------------------------------- parameters
def varied_frames(seed=6, n=24000, n_frames=2):
    """Frames that make sense under any geometry: ground over the whole range (denser near the sensor, gently undulating), a few
    boxes, a wall with its foot below the ground, a raised plateau, two raised rough patches in rings 2 and 3 and a rim beyond r = 60 with only a few points per patch."""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n_frames):
        r = 1.55 + 78.0 * rng.uniform(0, 1, n) ** 2
        th = rng.uniform(0, 2 * np.pi, n)
        z = GROUND_Z + 0.03 * np.sin(0.2 * r + k) + rng.normal(0, 0.02, n)
        g = np.stack([r * np.cos(th), r * np.sin(th), z, rng.uniform(0.3, 1.0, n)], 1)
        keep = (r < 60.0) | (rng.uniform(0, 1, n) < 0.03)          # a sparse rim: patches of one, two, three points
        rough = []                                                 # two default-geometry patches of rings 2 and 3, raised and rough all over
        for c, s in ((2, 3), (3, 4)):
            ss = 2 * np.pi / DEFAULT.ring_sectors[c]
            keep &= ~((r >= DEFAULT.ring_lo[c]) & (r < DEFAULT.ring_hi[c]) & (th >= s * ss) & (th < (s + 1) * ss))
            rough.append(patch_points(rng, 300, c, s, z0=GROUND_Z + 0.35, noise=0.05, th_frac=(0.0, 1.0), r_frac=(0.0, 1.0)))
        g = g[keep]
        boxes = [np.stack([cx + rng.uniform(-1, 1, 600), cy + rng.uniform(-0.8, 0.8, 600), rng.uniform(GROUND_Z, 0.0, 600), rng.uniform(0, 1, 600)], 1)
                 for cx, cy in ((6.0, 3.0), (-9.0, -4.0), (15.0, -12.0), (-25.0, 8.0))]
        plateau = np.stack([rng.uniform(-6, -4, 900), rng.uniform(3, 5, 900), GROUND_Z + 0.3 + rng.normal(0, 0.03, 900), rng.uniform(0.3, 1, 900)], 1)
        f = np.concatenate([g] + boxes + rough + [plateau, wall(rng, 1500, x=3.5 + 0.1 * k)]).astype(np.float32)
        frames.append(f[rng.permutation(len(f))])
    return frames


def _set(**kw):
    def tweak(p):
        for k, v in kw.items():
            if isinstance(v, (tuple, list)):
                for i, x in enumerate(v):
                    getattr(p, k)[i] = x
            else:
                setattr(p, k, v)
    return tweak


PARAMETER_SETS = {
    'num_iter_1': _set(num_iter=1),
    'num_lpr_1': _set(num_lpr=1),
    'num_lpr_above_patch': _set(num_lpr=100000),
    'num_min_pts_1': _set(num_min_pts=1),
    'two_rings_of_interest': _set(num_rings_of_interest=2),
    'no_ring_of_interest': _set(num_rings_of_interest=0),
    'one_ring_per_zone': _set(num_rings_each_zone=(1, 1, 1, 1)),
    'patches_418': _set(num_sectors_each_zone=(7, 13, 54, 31), num_rings_each_zone=(3, 2, 4, 5)),      # 418 = 6 * 64 + 34
    'patches_1024': _set(num_sectors_each_zone=(64, 64, 64, 64), num_rings_each_zone=(4, 4, 4, 4)),
}

# what vg_ground_create refuses, and vg_ground_reset has to refuse as well
REFUSED_SETS = {
    'sectors_65': _set(num_sectors_each_zone=(16, 65, 54, 32), num_rings_each_zone=(1, 1, 1, 1)),
    'sectors_0': _set(num_sectors_each_zone=(16, 32, 0, 32)),
    'patches_above_1024': _set(num_sectors_each_zone=(64, 64, 64, 64), num_rings_each_zone=(4, 4, 4, 5)),
    'rings_above_64': _set(num_sectors_each_zone=(1, 1, 1, 1), num_rings_each_zone=(16, 16, 16, 17)),
    'num_zones_3': _set(num_zones=3),
    'rings_of_interest_5': _set(num_rings_of_interest=5),
    'elevation_storage_1985': _set(max_elevation_storage=1985),
    'flatness_storage_1985': _set(max_flatness_storage=1985),
}
