"""Class lists of any length (clip.class_list, clip_utils.py:22-26, 43): vg_clip_scores_wide against the one-wave vg_clip_scores (same
bits up to 64 classes) and against float64 above, then through GraphClassifier, the pipeline against the CPU oracle and the fp16
default path.  The configuration checks at the top need no GPU.  `pytest -s` prints the largest errors."""
import ctypes

import numpy as np
import pytest
import torch

import clip_scores_ref as R

VG_OK, VG_ERR_ARG = 0, 1
EXTRA_MAPPED = ['Vehicle', 'Pedestrian', 'Cyclist', 'Background']


def _long_clip_cfg():
    """The shipped 24 classes plus `object 024` .. `object 099`, extra entry i mapped to EXTRA_MAPPED[i % 4]."""
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = default_preprocessor_cfg()
    extra = [f'object {i:03d}' for i in range(24, 100)]
    clip = dict(cfg['clip'])
    clip['class_list'] = list(clip['class_list']) + extra
    clip['class_mapping'] = {**clip['class_mapping'], **{name: EXTRA_MAPPED[i % 4] for i, name in enumerate(extra)}}
    cfg['clip'] = clip
    return cfg


# ------------------------------------------------------------------------------------------------------------------------- no GPU
def test_wide_entry_point_checks_its_arguments_before_any_launch():
    from vilgod_amd._lib import lib
    fn = lib.vg_clip_scores_wide
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)              # never dereferenced: every call below returns before a HIP call
    assert fn(None, 4, 512, p, 100, p, p, p, None) == VG_ERR_ARG
    assert fn(p, 4, 512, None, 100, p, p, p, None) == VG_ERR_ARG
    assert fn(p, 4, 512, p, 100, None, p, p, None) == VG_ERR_ARG
    assert fn(p, 4, 512, p, 100, p, None, p, None) == VG_ERR_ARG
    assert fn(p, 4, 512, p, 100, p, p, None, None) == VG_ERR_ARG
    assert fn(p, 4, 512, p, 0, p, p, p, None) == VG_ERR_ARG
    assert fn(p, 4, 512, p, -3, p, p, p, None) == VG_ERR_ARG
    assert fn(p, 0, 512, p, 100, p, p, p, None) == VG_OK
    assert fn(None, 0, 512, None, 0, None, None, None, None) == VG_OK


def test_class_list_validation_names_the_offending_classes():
    from vilgod_amd.clip_wrapper import validate_class_list
    clip = _long_clip_cfg()['clip']
    assert validate_class_list(clip['class_list'], clip['class_mapping']) == clip['class_list'] and len(clip['class_list']) == 100
    assert validate_class_list(clip['class_list']) == clip['class_list']
    mapping = {k: v for k, v in clip['class_mapping'].items() if k != 'object 057'}
    with pytest.raises(ValueError, match='object 057') as e:
        validate_class_list(clip['class_list'], mapping)
    assert 'class_mapping' in str(e.value) and 'object 056' not in str(e.value)
    twice = clip['class_list'][:70] + ['fire truck'] + clip['class_list'][70:]
    with pytest.raises(ValueError, match='fire truck') as e:
        validate_class_list(twice, clip['class_mapping'])
    assert 'class_list' in str(e.value)


def test_clip_wrapper_refuses_a_bad_class_list_at_construction():
    """Before the tower is built: no device is touched, so this runs on a host without one."""
    from vilgod_amd.clip_wrapper import ClipWrapper
    clip = _long_clip_cfg()['clip']
    mapping = {k: v for k, v in clip['class_mapping'].items() if k != 'object 031'}
    with pytest.raises(ValueError, match='object 031'):
        ClipWrapper(dict(clip, class_mapping=mapping), '/nonexistent', device='cpu')
    with pytest.raises(ValueError, match='wall'):
        ClipWrapper(dict(clip, class_list=clip['class_list'] + ['wall']), '/nonexistent', device='cpu')


# ------------------------------------------------------------------------------------------------------------------- kernel level
def _wide(feat, text, rows=None, fill=None):
    """lib.vg_clip_scores_wide on [n, D] features -> (probs, top1, score), allocated with `rows` >= n rows filled with `fill`."""
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    n, dim = feat.shape
    K = text.shape[0]
    rows = n if rows is None else rows
    probs = torch.full((rows, K), float('nan') if fill is None else fill[0], dtype=torch.float32, device=feat.device)
    top1 = torch.full((rows,), -7 if fill is None else fill[1], dtype=torch.int32, device=feat.device)
    score = torch.full((rows,), float('nan') if fill is None else fill[2], dtype=torch.float32, device=feat.device)
    check(lib.vg_clip_scores_wide(ptr(feat), n, dim, ptr(text), K, ptr(probs), ptr(top1), ptr(score), stream_ptr()), 'vg_clip_scores_wide')
    torch.cuda.synchronize()
    return probs, top1, score


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [512, 768])
@pytest.mark.parametrize('n_classes', [1, 2, 24, 63, 64])
def test_wide_returns_the_narrow_kernels_bits(cuda, dim, n_classes):
    """Up to 64 classes only wave 0 of the wide kernel owns classes and each of its steps is the one-wave kernel's."""
    from vilgod_amd._lib import lib, ptr, stream_ptr, check
    for scale in R.SCALES:
        feat, text = (t.to(cuda) for t in R.inputs(dim, n_classes, scale))
        probs = torch.full((R.N_CROPS, n_classes), float('nan'), device=cuda)
        top1 = torch.full((R.N_CROPS,), -7, dtype=torch.int32, device=cuda)
        score = torch.full((R.N_CROPS,), float('nan'), device=cuda)
        check(lib.vg_clip_scores(ptr(feat), R.N_CROPS, dim, ptr(text), n_classes, ptr(probs), ptr(top1), ptr(score), stream_ptr()), 'vg_clip_scores')
        p, t, s = _wide(feat, text)
        assert torch.equal(p, probs) and torch.equal(t, top1) and torch.equal(s, score), scale


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [512, 768, 100, 101, 7])
@pytest.mark.parametrize('n_classes', [65, 127, 128, 129, 255, 256, 257, 1000, 1025, 4097])
def test_wide_against_float64(cuda, dim, n_classes):
    """Class counts at lane, wave, workgroup-stride and tile edges; 100 columns end inside a column tile, 101 and 7 take the path
    of rows that are no whole 16-byte pieces.  The bars of tests/test_attention.py::test_clip_scores_shapes: |dp| <= 1e-5, top-1 equal
    where the reference's margin exceeds 2e-5, score == probs[top1] bit for bit, probs <= score.  (A float32 emulation of the
    sequential chain with unfused products stays at or below 2.7e-6 of float64 for 65 .. 4096 classes at all three scales.)"""
    from vilgod_amd.clip_wrapper import clip_scores
    worst = 0.0
    for scale in R.SCALES:
        feat, text, want = R.case(dim, n_classes, scale)
        probs, top1, score = (t.cpu() for t in clip_scores(feat.to(cuda), text.to(cuda)))
        err = float((probs.double() - want).abs().max())
        worst = max(worst, err)
        print(f'K {n_classes} D {dim} scale {scale:g}: max |dp| {err:.3e}')
        assert err <= 1e-5, scale
        R.check_top1(probs, top1, score, want)
        assert bool((top1 >= 0).all()) and bool((top1 < n_classes).all())
    print(f'K {n_classes} D {dim}: largest |dp| {worst:.3e} (bar 1e-5)')


@pytest.mark.gpu
def test_wide_text_table_off_16_byte_alignment(cuda):
    """A text table that starts 4 bytes past a 16-byte boundary is read float by float: the same bits as the aligned table."""
    feat, text = (t.to(cuda) for t in R.inputs(512, 129, 1.0))
    store = torch.empty(text.numel() + 1, device=cuda)
    shifted = store[1:].view(129, 512)
    shifted.copy_(text)
    assert shifted.data_ptr() % 16 == 4 and text.data_ptr() % 16 == 0
    a, b = _wide(feat, text), _wide(feat, shifted)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_wide_finds_the_winner_wherever_it_sits(cuda):
    winners = [0, 63, 64, 65, 255, 256, 257, 299]
    g = torch.Generator().manual_seed(R.seed('winner', 300))
    text = R.unit_rows(300, 512, g)
    feat = torch.randn(len(winners) + 3, 512, generator=g)
    for r, c in enumerate(winners):
        feat[r] = text[c]
    probs, top1, score = (t.cpu() for t in _wide(feat.to(cuda), text.to(cuda)))
    assert top1[:len(winners)].tolist() == winners
    want = R.reference(feat, text)
    assert float((probs.double() - want).abs().max()) <= 1e-5
    R.check_top1(probs, top1, score, want)


@pytest.mark.gpu
def test_wide_exact_ties(cuda):
    """Identical text rows in two waves (3, 200), across the wave edge (63, 64) and across the workgroup stride (255, 256: the last
    thread's first class and the first thread's second): the same bits in both columns, and the lower index wins where the pair is
    the best."""
    pairs = [(3, 200), (63, 64), (255, 256)]
    g = torch.Generator().manual_seed(R.seed('ties', 300))
    text = R.unit_rows(300, 512, g)
    for lo, hi in pairs:
        text[hi] = text[lo]
    feat = torch.randn(8 * len(pairs) + 8, 512, generator=g)
    for k, (lo, hi) in enumerate(pairs):                                   # 8 rows per pair whose best class is that pair
        rows = slice(8 * k, 8 * k + 8)
        feat[rows] += 3.0 * text[lo] * feat[rows].norm(dim=-1, keepdim=True)
    want = R.reference(feat, text)
    probs, top1, score = (t.cpu() for t in _wide(feat.to(cuda), text.to(cuda)))
    assert float((probs.double() - want).abs().max()) <= 1e-5
    for k, (lo, hi) in enumerate(pairs):
        rows = slice(8 * k, 8 * k + 8)
        assert torch.equal(probs[:, lo], probs[:, hi])
        assert bool((top1[rows] == lo).all()) and bool((top1 != hi).all())
        assert torch.equal(score[rows], probs[rows, lo])


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_classes', [(512, 24), (512, 65), (100, 257), (101, 1025)])
def test_wide_writes_only_its_rows(cuda, dim, n_classes):
    """Outputs allocated with one row more than the call has crops: the canaries of that row survive; n = 0 writes nothing at all."""
    feat, text = (t.to(cuda) for t in R.inputs(dim, n_classes, 1.0))
    fill = (-123.0, -9, -456.0)
    probs, top1, score = _wide(feat, text, rows=R.N_CROPS + 1, fill=fill)
    assert bool((probs[-1] == fill[0]).all()) and int(top1[-1]) == fill[1] and float(score[-1]) == fill[2]
    assert bool((probs[:-1] >= 0).all()) and bool((top1[:-1] >= 0).all())
    probs, top1, score = _wide(feat[:0], text, rows=2, fill=fill)
    assert bool((probs == fill[0]).all()) and bool((top1 == fill[1]).all()) and bool((score == fill[2]).all())


# ------------------------------------------------------------------------------------------------------------ through the layers
@pytest.mark.gpu
def test_graph_classifier_takes_100_classes(cuda):
    """vg_vit_classify_graph with a 100-row text table: 8 crops twice.  A handle's first call runs as plain launches (it sets the
    kernels' attributes), the second captures the graph and replays it: both equal the plain encode + clip_scores exactly."""
    from vilgod_amd import clip_weights as cw
    from vilgod_amd.clip_wrapper import VitEncoder, GraphClassifier, clip_scores
    text = cw.synthetic_text_features(6, 100, 512).to(cuda)
    enc = VitEncoder(cw.synthetic_vit_weights(0, **cw.VIT_B16), dtype='f16', device=cuda)
    plain = enc.view()
    g = GraphClassifier(enc, text, max_crops=8, patch_width=256)
    n, rows = 8, (8 * 196 + 255) // 256 * 256
    p = (torch.randint(0, 256, (rows, 256), generator=torch.Generator().manual_seed(11)).float() / 256.0).half().to(cuda)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        g.patch_buffer(n)[:rows].copy_(p)
        got = []
        for _ in range(2):
            got.append([t.clone() for t in g.classify(n)])
            g.probs.fill_(-1.0)                                # the second call has to write its own results
        want = clip_scores(plain.encode_patches(p, n), text)
        stream.synchronize()
    assert want[0].shape == (8, 100)
    for probs, top1, score in got:
        assert torch.equal(probs, want[0]) and torch.equal(top1, want[1]) and torch.equal(score, want[2])
    st = g.stats()
    assert st['graphs_captured'] == 1 and st['graph_launches'] == 1, st


@pytest.mark.gpu
def test_pipeline_matches_oracle_with_100_classes(cuda):
    """tests/test_pipeline.py::test_pipeline_matches_oracle_20k with a 100-entry class list: same frame, poses and arguments; text
    features of seed 6, whose winners lie on both sides of class 64 and map to two names (seed 0 sends every crop to class 80)."""
    from vilgod_amd import synthetic, clip_weights as cw
    from vilgod_amd.pipeline import PseudoLabelPipeline
    from oracle.pipeline_oracle import OraclePipeline
    cfg = _long_clip_cfg()
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    pipe = PseudoLabelPipeline(cfg, device=cuda, vit_dtype='f32', max_points=25_000, clip_model_path='/nonexistent',
                               angle_mode='reference')
    text = cw.synthetic_text_features(6, 100, 512)
    assert pipe.clip.text_features.shape == (100, 512)
    pipe.clip.text_features = text.to(cuda).contiguous()
    fs, res = pipe.process_frame(pts, poses[1], poses[0], fnr=1)
    orc = OraclePipeline(cw.synthetic_vit_weights(0, **cw.VIT_B16), text, cfg['clip']['class_list'], cfg['clip']['class_mapping'],
                         box_all_edges=False)
    o = orc.process_frame(pts, poses[1], poses[0])
    assert np.array_equal(fs.valid, o['valid'])
    want_p = np.asarray(o['probs_clip'])
    winners = want_p.argmax(-1)
    top2 = np.sort(want_p, axis=-1)[:, -2:]
    print('valid', int(o['valid'].sum()), 'crops', len(winners), 'winning classes', sorted(set(winners.tolist())),
          'smallest top-1 margin', float((top2[:, 1] - top2[:, 0]).min()))
    assert (winners >= 64).any() and (winners < 64).any()                  # the generators still put winners on both kernels' ground
    got_p = pipe.last_probs.cpu().numpy()
    assert got_p.shape == want_p.shape and got_p.shape == (4 * int(o['valid'].sum()), 100)
    err = np.abs(got_p - want_p).max()
    print('max |dp|', err)
    assert err < 1e-3
    e = fs.cls[pipe.cls_key]
    rows = np.flatnonzero(fs.valid)
    assert [str(e['name'][r]) for r in rows] == list(o['names'])
    assert len(set(o['names'])) >= 2
    assert np.abs(np.array([e['final'][r] for r in rows], np.float64) - np.array(o['scores'], np.float64)).max() < 1e-3
    assert len(res['name']) == len(res['score']) == len(res['boxes_lidar'])


@pytest.mark.gpu
def test_fp16_graph_path_classifies_100_classes(cuda):
    """The default fp16 path with vit_graph on a worker stream and the 100-entry list: (probs, top1, score) of pipe.classify -- the
    handle's first call (plain launches) and the second (captured) -- equal clip_scores(encode_patches(rows)) of the same renderer's
    rows exactly."""
    from vilgod_amd import synthetic
    from vilgod_amd.clip_wrapper import clip_scores
    from vilgod_amd.frame_state import pack_clusters
    from vilgod_amd.pipeline import PseudoLabelPipeline
    pipe = PseudoLabelPipeline(_long_clip_cfg(), device=cuda, vit_dtype='f16', max_points=25_000, clip_model_path='/nonexistent',
                               box_workers=0, box_mode='fast', vit_graph=True)
    assert pipe.clip.text_features.shape == (100, 512)
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fs, d_ref, d_X, gidx = pipe.prepare(pts, poses[1], poses[0])
    labels, probs = pipe.cluster(d_X)
    _, index, seg = pack_clusters(labels, probs, pipe.prob_threshold)
    C = min(8, len(seg) - 1)
    assert C >= 2
    d_seg = torch.from_numpy(np.ascontiguousarray(seg[:C + 1], np.int32)).to(cuda)
    d_index = torch.from_numpy(np.ascontiguousarray(index[:seg[C]], np.int32)).to(cuda)
    n = C * pipe.projection.num_views
    stream = torch.cuda.Stream(device=cuda)
    stream.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(stream):
        got = [pipe.classify(d_X, d_index, d_seg, fs.transform_to_ego) for _ in range(2)]
        patches = pipe.projection.render_frame(d_X, d_index, d_seg, fs.transform_to_ego, out='patch16c1' if pipe.patch_1ch else 'patch16')
        want = clip_scores(pipe.clip.encoder.encode_patches(patches, n), pipe.clip.text_features)
        stream.synchronize()
    assert pipe._graph_cls is not None and pipe._graph_cls.stats()['graphs_captured'] == 1
    assert want[0].shape == (n, 100)
    for p, t, s in got:
        assert torch.equal(p, want[0]) and torch.equal(t, want[1]) and torch.equal(s, want[2])
