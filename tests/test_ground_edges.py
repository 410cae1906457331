"""csrc/ground.hip at the branches its ordinary inputs never reach: TGR, R-VPF, threshold stores that fill, evict and wrap, the
patch-size thresholds of k_pw_patch / k_pw_sort_big, exact binning edges, non-default parameters and geometries, row strides,
vg_ground_reset's validation.

Two halves.  The CPU tests run the oracle alone and assert, from its reach counters (oracle.counts()), that every scene of
tests/ground_ref.py reaches the branch it was built for and that the branch changes the answer.  The GPU tests then assert the
one equality of tests/test_ground.py -- ground set, adaptive state and patch records equal the oracle's, frame after frame -- on
those scenes.
"""
import ctypes
import functools

import numpy as np
import pytest

import ground_ref as gr
from ground_ref import _same_sequence, same_frame
from oracle import patchworkpp as opw


@functools.lru_cache(maxsize=None)
def tgr_frames():
    return gr.tgr_scene()


@functools.lru_cache(maxsize=None)
def rvpf_frames(n_patch, wall_x=4.0):
    return gr.rvpf_scene(n_patch, wall_x=wall_x, with_wall_only_patch=wall_x < 11)


# name -> (frames, parameter tweak, storage limit)
def _storage(limit, base=None):
    def tweak(p):
        if base:
            base(p)
        p.max_elevation_storage = p.max_flatness_storage = limit
    return tweak


STORE_RUNS = {
    'default_88_frames': (lambda: gr.store_frames(88), None, 1000),
    'sectors64_40_frames': (lambda: gr.store_frames(40, gr.GEOM64, per_patch=20), gr.sectors64, 1000),
    'sectors64_storage_1984': (lambda: gr.store_frames(40, gr.GEOM64, per_patch=20), _storage(1984, gr.sectors64), 1984),
    'storage_40': (lambda: gr.store_frames(8), _storage(40), 40),
}


@functools.lru_cache(maxsize=None)
def store_run(name):
    make, tweak, limit = STORE_RUNS[name]
    return make(), tweak, limit


@functools.lru_cache(maxsize=None)
def varied():
    return gr.varied_frames()


def _total(counts, group):
    return {k: sum(c[group][k] for c in counts) for k in counts[0][group]}


def _differ(frames, tweak):
    on, counts, _ = gr.oracle_masks(frames)
    off, _, _ = gr.oracle_masks(frames, tweak)
    return [int((a ^ b).sum()) for a, b in zip(on, off)], counts


# ------------------------------------------------------------------------------------------- CPU: the scenes reach their branches
def test_scene_tgr_reaches_every_outcome():
    frames = tgr_frames()
    diff, counts = _differ(frames, gr.tgr_off)
    tgr, gle = _total(counts, 'tgr'), _total(counts, 'gle')
    carry, after_clear = sum(c['rings_carry'] for c in counts), sum(c['rings_after_clear'] for c in counts)
    print(f'tgr scene: points that enable_TGR decides per frame {diff}; outcomes {tgr}; GLE {gle}; rings with carried flatness {carry}, '
          f'rings right after a clearing ring {after_clear}')
    assert diff[1] >= 50 and diff[2] >= 50
    assert all(v >= 1 for v in tgr.values()), tgr
    assert gle['candidate'] >= 4 and gle['near_by_elevation'] >= 1 and gle['near_by_flatness'] >= 1 and gle['far_accepted'] >= 1
    assert gle['heading_inside'] >= 1
    assert carry >= 1 and after_clear >= 1
    # candidates in zone 0 (rings 0, 1: 16 sectors) and in the near rings of zone 1 (rings 2, 3: 32 sectors)
    o = gr.oracle_for()
    per_ring = np.zeros(4, int)
    for f in frames:
        opw.mask_ground_points(f, o, 0.0)
        info = o.patch_info()
        for c in range(4):
            b = gr.DEFAULT.ring_base[c]
            per_ring[c] += int((info[b:b + gr.DEFAULT.ring_sectors[c], 11] == 2).sum())
    print('tgr scene: candidates per near ring', per_ring.tolist())
    assert (per_ring >= 1).all()
    # the `> 1500` rule and the line_variable veto meet what they are about
    big = [(c, s) for c in range(4) for s in range(gr.DEFAULT.ring_sectors[c]) if info[gr.DEFAULT.pid(c, s), 11] == 2 and info[gr.DEFAULT.pid(c, s), 1] > 1500]
    assert big and all(info[gr.DEFAULT.pid(c, s), 8:11].min() < 0.125 ** 2 for c, s in big)
    # with TGR off nothing is a TGR outcome, and the scene still has its candidates
    off = gr.oracle_masks(frames, gr.tgr_off)[1]
    assert sum(_total(off, 'tgr').values()) == 0 and _total(off, 'gle')['candidate'] >= 4


@pytest.mark.parametrize('n_patch,lo,hi', [(1000, 0, 4096), (3000, 4096, 16384), (15000, 16384, 10 ** 9)])
def test_scene_rvpf_wall_below_ground(n_patch, lo, hi):
    frames = rvpf_frames(n_patch)
    diff, counts = _differ(frames, gr.rvpf_off)
    size = int(gr.oracle_masks(frames)[0][0].size)
    o = gr.oracle_for()
    opw.mask_ground_points(frames[0], o, 0.0)
    n = int(o.patch_info()[gr.DEFAULT.pid(0, 0), 0])
    print(f'rvpf scene ({size} points, wall patch {n}): enable_RVPF decides {diff[0]} points; patches with removals '
          f'{counts[0]["rvpf_patches"]}, points removed {counts[0]["rvpf_killed"]}')
    assert lo < n <= hi and n == n_patch + 3000
    assert diff[0] >= 50
    assert counts[0]['rvpf_patches'] >= 2 and counts[0]['rvpf_killed'] >= 1000      # the wall patch and the patch that is only wall
    assert gr.oracle_masks(frames, gr.rvpf_off)[1][0]['rvpf_killed'] == 0


def test_scene_rvpf_wall_in_zone_1_is_fitted_once_and_kept():
    frames = rvpf_frames(1000, 12.5)
    _, counts, _ = gr.oracle_masks(frames)
    print('rvpf zone-1 scene:', {k: counts[0][k] for k in ('rvpf_far_vertical', 'rvpf_patches', 'rvpf_killed')})
    assert counts[0]['rvpf_far_vertical'] >= 1 and counts[0]['rvpf_killed'] == 0


@pytest.mark.parametrize('name', list(STORE_RUNS))
def test_scene_stores_fill_evict_and_wrap(name):
    frames, tweak, limit = store_run(name)
    _, counts, states = gr.oracle_masks(frames, tweak)
    appended = counts[-1]['appended']
    ev_e = np.array([c['evicted_elev'] for c in counts])
    ev_f = np.array([c['evicted_flat'] for c in counts])
    n_max = np.max([s['n_elevation'] for s in states], 0)
    thr = np.array([s['elevation_thr'] for s in states])
    print(f'stores {name}: {len(frames)} frames of {len(frames[0])} points; appended {appended.tolist()}; frames that evict '
          f'elevation {(ev_e > 0).sum(0).tolist()} flatness {(ev_f > 0).sum(0).tolist()}; largest store {n_max.tolist()}')
    assert (n_max == limit).all()                                       # all four stores fill
    assert ((ev_e > 0).sum(0) >= (5 if name == 'storage_40' else 8 if limit == 1984 else 10)).all()
    assert np.array_equal(ev_e > 0, ev_f > 0)
    if name == 'storage_40':
        assert (ev_e[2] > 0).any()                                      # eviction from the third frame
    else:
        assert (n_max > 512).all()                                      # summed in more than one 512-value chunk
        wrapping = [2, 3] if name == 'default_88_frames' else [0, 1, 2, 3]
        assert (appended[wrapping] > 2048).all()
        # ... and already before the last three frames, which run after the state handoff
        assert (counts[-4]['appended'][wrapping] > 2048).all()
    assert len(np.unique(thr[len(thr) // 2:, 0])) > len(thr) // 4       # the thresholds keep moving


def test_scene_patch_sizes_are_exact():
    frames = gr.patch_size_scene()
    slots = gr.patch_size_slots()
    o = gr.oracle_for()
    for f in frames:
        opw.mask_ground_points(f, o, 0.0)
        info = o.patch_info()
        got = {n: int(info[gr.DEFAULT.pid(c, s), 0]) for n, (c, s) in slots.items()}
        assert all(n == v for n, v in got.items()), got
        assert info[gr.DEFAULT.pid(*slots[9]), 1] == 0 and info[gr.DEFAULT.pid(*slots[10]), 1] > 0      # num_min_pts = 10
        # ties at the lowest z straddle the seed cut: more than num_lpr = 20 points share the minimum
        for n, (c, s) in slots.items():
            if n >= 63:
                ang = (np.arctan2(f[:, 1].astype(np.float64), f[:, 0].astype(np.float64)) % (2 * np.pi)) // (2 * np.pi / 16)
                r = np.hypot(f[:, 0].astype(np.float64), f[:, 1].astype(np.float64))
                z = f[(ang == s) & (r < gr.DEFAULT.ring_hi[0]), 2]
                assert len(z) == n and (z == z.min()).sum() > 20 and len(np.unique(z)) < n // 2
    print('patch sizes:', sorted(got.values()), 'points', len(frames[0]), 'counters', o.counts()['gle'])
    assert not np.array_equal(frames[0], frames[1]) and np.array_equal(np.sort(frames[0][:, 2]), np.sort(frames[1][:, 2]))


def _expected_bin(x, y, g=gr.DEFAULT, min_range=1.5, max_range=80.0):
    """The patch of (x, y) by concentric_idx / sector arithmetic in float64 (patchworkpp.cpp:569-623), or None outside the range."""
    r = np.sqrt(np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y))
    if not (r <= max_range and r > min_range):
        return None
    theta = np.arctan2(np.float64(y), np.float64(x))
    if not theta > 0:
        theta = 2 * np.pi + theta
    z = g.zone_bounds
    zone = 0 if r < z[1] else 1 if r < z[2] else 2 if r < z[3] else 3
    ring = min(int((r - z[zone]) / ((z[zone + 1] - z[zone]) / g.rings[zone])), g.rings[zone] - 1)
    sector = min(int(theta / (2 * np.pi / g.sectors[zone])), g.sectors[zone] - 1)
    return g.pid(sum(g.rings[:zone]) + ring, sector)


def test_scene_binning_edges_fall_where_the_arithmetic_says():
    frames, n_ground, n_edge = gr.binning_scene()
    edge = frames[0][n_ground:]
    want = np.full(gr.DEFAULT.n_patches, 24)
    n_in = 0
    with np.errstate(invalid='ignore'):
        for x, y, z, _ in edge:
            b = None if (np.isnan(z) or z == np.finfo(np.float32).tiny) else _expected_bin(x, y)
            if b is not None:
                want[b] += 1
                n_in += 1
    # 9 radii x 8 half-axis points, 2 radii out of range; the NaN / inf / FLT_MIN points are out
    assert n_in == 7 * 8 and n_edge == 72 + 9
    # on the half-axes the angle is a multiple of pi / 2: sector boundaries for 16 and 32 sectors, theta = 2 pi clamps to the last one
    assert _expected_bin(5.0, -0.0) == gr.DEFAULT.pid(0, 15) and _expected_bin(5.0, 0.0) == gr.DEFAULT.pid(0, 15)
    assert _expected_bin(0.0, 5.0) == gr.DEFAULT.pid(0, 4) and _expected_bin(-5.0, -0.0) == gr.DEFAULT.pid(0, 8) and _expected_bin(-0.0, -5.0) == gr.DEFAULT.pid(0, 12)
    assert _expected_bin(11.3125, 0.0) == gr.DEFAULT.pid(2, 31) and _expected_bin(0.0, 21.125) == gr.DEFAULT.pid(6, 13) and _expected_bin(80.0, 0.0) == gr.DEFAULT.pid(13, 31)
    o = gr.oracle_for()
    for f in frames:
        with np.errstate(invalid='ignore'):
            idx = opw.mask_ground_points(f, o, 0.0)
        assert np.array_equal(o.patch_info()[:, 0].astype(int), want)
    print('binning scene: edge points in range', n_in, 'of', n_edge, '; patches holding one or more of them', int((want > 24).sum()))
    m = np.zeros(len(frames[1]), bool)
    m[idx] = True
    assert not m[:n_edge][-9:].any() and m[n_edge:].mean() > 0.9


def test_scene_single_stored_value():
    _, counts, states = gr.oracle_masks(gr.single_value_scene())
    print('single-value scene: appended', counts[0]['appended'].tolist(), 'state', states[0]['sensor_height'], states[0]['elevation_thr'].tolist())
    assert counts[0]['appended'].tolist() == [1, 0, 0, 0] and counts[0]['gle']['near_by_elevation'] == 1
    assert states[0]['n_elevation'].tolist() == [1, 0, 0, 0]
    assert states[0]['sensor_height'] == 0 and np.signbit(states[0]['sensor_height']) and states[0]['elevation_thr'][0] == 0
    assert counts[1]['appended'].tolist() == [17, 16, 32, 32] and states[1]['sensor_height'] > 1.6


@pytest.mark.parametrize('name', list(gr.PARAMETER_SETS))
def test_scene_parameter_sets(name):
    frames, tweak = varied(), gr.PARAMETER_SETS[name]
    masks, counts, states = gr.oracle_masks(frames, tweak)
    base = gr.oracle_masks(frames)[0]
    o = gr.oracle_for(tweak=tweak)
    opw.mask_ground_points(frames[0], o, 0.0)
    sizes = o.patch_info()[:, 0]
    print(f'parameters {name}: {len(sizes)} patches, ground {[int(m.sum()) for m in masks]}, differs from the defaults in '
          f'{[int((a ^ b).sum()) for a, b in zip(masks, base)]} points; GLE {counts[1]["gle"]}; removed by R-VPF {counts[1]["rvpf_killed"]}')
    assert all(m.mean() > 0.5 for m in masks)
    assert np.isfinite(states[1]['elevation_thr']).all() and np.isfinite(states[1]['flatness_thr']).all()
    assert any((a ^ b).any() for a, b in zip(masks, base))                    # the setting decides something on these frames
    if name == 'num_min_pts_1':
        assert (sizes == 1).any() and ((sizes > 1) & (sizes < 10)).any()
    if name == 'num_lpr_above_patch':
        assert sizes.max() < 100000
    if name == 'patches_418':
        assert len(sizes) == 418 and len(sizes) % 64
    if name == 'patches_1024':
        assert len(sizes) == 1024
    if name == 'one_ring_per_zone':
        assert len(sizes) == 16 + 32 + 54 + 32


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('tgr', [1, 0])
def test_hip_ground_tgr(cuda, tgr):
    """Every TGR outcome (reverted by the sigmoid / by the > 1500 rule, rejected by the sigmoid / by line_variable), candidates in
    zone 0 and zone 1, statistics carried over candidate-free rings and cleared by rings with candidates; and the same with TGR off."""
    _same_sequence(tgr_frames(), 0.0, cuda, tweak=None if tgr else gr.tgr_off)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['lds_4000', 'big_6000', 'big_18000', 'zone_1', 'rvpf_off'])
def test_hip_ground_rvpf(cuda, case):
    """A wall whose foot is below the ground: R-VPF removes points and refits over the survivors, with the alive flags in LDS
    (4000-point patch) and in inlier[] == 2 (6000: keys sorted in LDS, 18000: sorted in global memory); in zone 1 it fits once
    and removes nothing."""
    frames = {'lds_4000': rvpf_frames(1000), 'big_6000': rvpf_frames(3000), 'big_18000': rvpf_frames(15000),
              'zone_1': rvpf_frames(1000, 12.5), 'rvpf_off': rvpf_frames(1000)}[case]
    _same_sequence(frames, 0.0, cuda, tweak=gr.rvpf_off if case == 'rvpf_off' else None)


def _blob_cursors(blob):
    """elev_head, elev_cnt, flat_head, flat_cnt of an exported state (behind sensor_height and the eight thresholds)."""
    c = np.frombuffer(blob, dtype=np.int32, count=16, offset=9 * 8).reshape(4, 4)
    return c[0], c[1], c[2], c[3]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(STORE_RUNS))
def test_hip_ground_stores(cuda, name):
    """The threshold stores past their limits.  Lengths and what the oracle's counters show for them (test_scene_stores_...):
      default_88_frames       88 frames x 3840 points: appended 1405/1383/2668/2686 values per ring, all four stores reach 1000 (two
                              chunks), eviction on 26/25/56/55 frames, rings 2 and 3 pass 2048 appended values: their cursors wrap
      sectors64_40_frames     40 frames x 5120 points, 896 patches: appended 2542/2436/2445/2449, every store wraps, eviction on 24-25 frames
      sectors64_storage_1984  the same frames with the largest limits vg_ground_create accepts: appended 2543/2446/2449/2451, the stores
                              reach 1984 (four chunks, up to 2048 values in the buffer before eviction), eviction on 8-9 frames
      storage_40              8 frames x 3840 points, limits of 40: appended 128/125/232/220, eviction on 6/6/7/7 frames, from the second
                              or third frame on
    The last three frames run after the state went through export_state / set_state onto a fresh handle: they must equal the
    oracle's, and both handles' states byte for byte."""
    from vilgod_amd import patchworkpp as gpw
    frames, tweak, limit = store_run(name)
    gpu, oracle = _same_sequence(frames[:-3], 0.0, cuda, tweak=tweak, return_oracle=True)
    blob = gpu.export_state()
    # the ring cursors are where the oracle's tallies put them: head = values evicted so far, modulo the capacity
    appended = oracle.counts()['appended']
    e_head, e_cnt, f_head, f_cnt = _blob_cursors(blob)
    assert np.array_equal(e_cnt, oracle.state()['n_elevation']) and np.array_equal(f_cnt, oracle.state()['n_flatness'])
    assert np.array_equal(e_head, (appended - e_cnt) % 2048) and np.array_equal(f_head, (appended - f_cnt) % 2048)
    pg = gpw.Parameters()
    pg.min_range = 1.5
    if tweak:
        tweak(pg)
    other = gpw.patchworkpp(pg, max_points=len(frames[0]) + 1, device=cuda)
    other.set_state(blob)
    for k, f in enumerate(frames[-3:]):
        same_frame(oracle, gpu, f, 0.0, k)
        got = np.sort(gpw.mask_ground_points_patchwork_pp(f, other, 0.0))
        assert np.array_equal(got, np.flatnonzero(oracle.ground_mask())), k
    assert other.export_state() == gpu.export_state()


@pytest.mark.gpu
def test_hip_ground_patch_sizes(cuda):
    """Patches of exactly 9, 10, 11, 63 ... 16385 points (num_min_pts, the padding of the bitonic network, the 4096 and 16384
    thresholds between the three sort paths), z with exact ties across the seed cut, in two point orders."""
    _same_sequence(gr.patch_size_scene(), 0.0, cuda)


@pytest.mark.gpu
def test_hip_ground_binning_edges(cuda):
    frames, _, _ = gr.binning_scene()
    _same_sequence(frames, 0.0, cuda)


@pytest.mark.gpu
def test_hip_ground_single_stored_value(cuda):
    gpu = _same_sequence(gr.single_value_scene()[:1], 0.0, cuda)
    s = gpu.state()
    assert s['n_elevation'].tolist() == [1, 0, 0, 0] and s['elevation_thr'][0] == 0 and np.signbit(s['sensor_height'])
    _same_sequence(gr.single_value_scene(), 0.0, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(gr.PARAMETER_SETS))
def test_hip_ground_parameter_sets(cuda, name):
    _same_sequence(varied(), 0.0, cuda, tweak=gr.PARAMETER_SETS[name])


@pytest.mark.gpu
def test_hip_ground_row_stride(cuda):
    """Rows of 5 and 7 floats with garbage behind the four columns: the same answer as rows of 4."""
    import torch
    from vilgod_amd import patchworkpp as gpw
    pts = varied()[0].copy()
    pts[:, 2] += np.float32(1.723)
    ref, oracle = _same_sequence([pts], 1.723, cuda, return_oracle=True)          # rows of 4: the oracle's answer
    want = np.flatnonzero(oracle.ground_mask())
    assert len(want) > len(pts) // 2
    p = gpw.Parameters()
    p.min_range = 1.5
    rng = np.random.default_rng(0)
    for stride in (5, 7):
        rows = rng.uniform(-1e30, 1e30, (len(pts), stride)).astype(np.float32)
        rows[::3, 4:] = np.nan
        rows[:, :4] = pts
        t = torch.from_numpy(rows).to(cuda)
        assert t.stride(0) == stride
        h = gpw.patchworkpp(p, max_points=len(pts), device=cuda)
        got = np.sort(gpw.mask_ground_points_patchwork_pp(t, h, 1.723))
        assert np.array_equal(got, want), stride
        assert h.export_state() == ref.export_state() and np.array_equal(h.patch_info(), ref.patch_info(), equal_nan=True)


def _small_frames():
    rng = np.random.default_rng(7)
    return [gr.ground(rng, 40, gr.NEAR) for _ in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(gr.REFUSED_SETS))
def test_hip_ground_reset_refuses_what_create_refuses(cuda, name):
    from vilgod_amd import patchworkpp as gpw
    from vilgod_amd._lib import lib
    frames = _small_frames()
    gpu, oracle = _same_sequence(frames[:1], 0.0, cuda, return_oracle=True)
    bad = gpw.Parameters()
    bad.min_range = 1.5
    gr.REFUSED_SETS[name](bad)
    h = ctypes.c_void_p()
    assert lib.vg_ground_create(ctypes.byref(h), ctypes.byref(bad), 1000) == 1          # the argument error, nothing created
    # the return code first: no frame may run on a handle that took such parameters
    assert lib.vg_ground_reset(gpu._h, ctypes.byref(bad)) == 1
    assert lib.vg_ground_num_patches(gpu._h) == 504
    with pytest.raises(Exception):
        gpu.reset(bad)
    assert gpu._params is not bad
    same_frame(oracle, gpu, frames[1], 0.0, 1)                    # previous parameters, and the sequence goes on
    same_frame(oracle, gpu, frames[2], 0.0, 2)


@pytest.mark.gpu
def test_hip_ground_reset_to_another_geometry(cuda):
    """A valid reset to another geometry behaves like a fresh handle of that geometry."""
    from vilgod_amd import patchworkpp as gpw
    frames = gr.store_frames(3, gr.GEOM64, per_patch=14)          # 3584 points: within the first handle's capacity
    gpu = _same_sequence(_small_frames(), 0.0, cuda)
    p = gpw.Parameters()
    p.min_range = 1.5
    gr.sectors64(p)
    gpu.reset(p)
    assert gpu.patch_info().shape[0] == 896
    fresh = _same_sequence(frames, 0.0, cuda, tweak=gr.sectors64)
    oracle = gr.oracle_for(tweak=gr.sectors64)
    for k, f in enumerate(frames):
        same_frame(oracle, gpu, f, 0.0, k)
    assert gpu.export_state() == fresh.export_state()
    gpu.reset()                                                   # no parameters: the geometry stays, the state starts over
    same_frame(gr.oracle_for(tweak=gr.sectors64), gpu, frames[0], 0.0)
