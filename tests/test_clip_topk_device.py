"""vg_clip_topk (csrc/clip_topk.hip) on the GPU: the kernel against its host twin on the crafted tables of tests/clip_topk_ref.py, behind
the two score kernels (column 0 = their top-1 on every bit), behind the captured classification (GraphClassifier), through the pipeline
and the command line with clip.top_k = 3, and captured into a graph by itself.  Every comparison is of bits."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import clip_topk_ref as R
from conftest import ROOT
from vilgod_amd import clip_weights as cw, synthetic

pytestmark = pytest.mark.gpu
KEY = 'clip_a_point_representation_of_a'


def _device(table, k, cuda, n=None):
    """vg_clip_topk on sentinel-filled outputs with one guard row behind them -> (idx, score) whole buffers on the host"""
    from vilgod_amd.clip_wrapper import clip_topk
    n = len(table) if n is None else n
    d = torch.from_numpy(np.ascontiguousarray(table[:n])).to(cuda)
    idx = torch.full((n + 1, k), int(R.SENTINEL_I), dtype=torch.int32, device=cuda)
    score = torch.full((n + 1, k), float(R.SENTINEL_F), dtype=torch.float32, device=cuda)
    top, sc = clip_topk(d, k, idx, score)
    assert top.shape == (n, k) and sc.shape == (n, k)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy()


# ---- host twin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', R.SIZES_K)
def test_kernel_equals_its_host_twin_on_crafted_tables(cuda, K):
    from vilgod_amd._lib import lib
    names, table = R.crafted_table(K)
    for k in R.ks_for(K):
        for n in (len(table), 0, 1, 3):
            st, h_idx, h_score = R.host(lib, table[:n], k)
            assert st == 0
            d_idx, d_score = _device(table, k, cuda, n)
            assert np.array_equal(d_idx, h_idx), (K, k, n, [names[r] for r in np.unique(np.argwhere(d_idx != h_idx)[:, 0])[:5] if r < len(names)])
            assert np.array_equal(R.bits(d_score), R.bits(h_score)), (K, k, n)       # the guard row's sentinels included
            assert np.all(d_idx[n:] == R.SENTINEL_I) and np.all(d_score[n:] == R.SENTINEL_F)
            assert not np.any(d_idx[:n] == R.SENTINEL_I)                                # every slot written


def test_device_refusals_launch_nothing(cuda):
    from vilgod_amd._lib import lib, ptr, stream_ptr
    table = torch.from_numpy(R.crafted_table(64)[1][:3]).to(cuda)
    idx = torch.full((3, 5), int(R.SENTINEL_I), dtype=torch.int32, device=cuda)
    score = torch.full((3, 5), float(R.SENTINEL_F), dtype=torch.float32, device=cuda)
    for k, K, null in ((0, 64, ()), (-1, 64, ()), (33, 64, ()), (5, 4, ()), (1, 0, ()), (1, -3, ()), (2, 64, ('probs',)), (2, 64, ('idx',)),
                       (2, 64, ('score',))):
        p = lambda t, name: None if name in null else ptr(t)
        assert lib.vg_clip_topk(p(table, 'probs'), 3, K, k, p(idx, 'idx'), p(score, 'score'), stream_ptr()) == 1, (k, K, null)
    assert lib.vg_clip_topk(None, 0, 64, 2, None, None, stream_ptr()) == 0 and lib.vg_clip_topk(ptr(table), -1, 64, 2, ptr(idx), ptr(score), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((idx == int(R.SENTINEL_I)).all()) and bool((score == float(R.SENTINEL_F)).all())


# ---- behind the score kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [512, 768])
@pytest.mark.parametrize('K', [24, 64, 65, 257, 1203])
def test_column_0_is_the_score_kernels_top1(cuda, K, D):
    from vilgod_amd.clip_wrapper import clip_scores
    n = 33
    gen = torch.Generator().manual_seed(K + D)
    feat = (torch.randn(n, D, generator=gen) * 1.3).to(cuda)
    text = cw.synthetic_text_features(K, K, D).to(cuda)
    probs1, top1, score1 = clip_scores(feat, text)
    for k in R.ks_for(K)[1:]:
        probs, top, score = clip_scores(feat, text, top_k=k)
        torch.cuda.synchronize()
        assert top.shape == (n, k) and top.dtype == torch.int32 and score.shape == (n, k) and score.dtype == torch.float32
        assert torch.equal(probs.view(torch.int32), probs1.view(torch.int32))
        assert torch.equal(top[:, 0], top1) and torch.equal(score[:, 0].contiguous().view(torch.int32), score1.view(torch.int32))
        want_idx, want_score = R.order(probs.cpu().numpy(), k)
        assert np.array_equal(top.cpu().numpy(), want_idx), (K, D, k)
        assert np.array_equal(R.bits(score.cpu().numpy()), R.bits(want_score))
    assert clip_scores(feat, text, top_k=1)[1].shape == (n,)                            # top_k = 1: today's shapes
    with pytest.raises(ValueError, match=r'clip\.top_k'):
        clip_scores(feat, text, top_k=K + 1 if K < 32 else 33)


# ---- the captured classification -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clips(cuda):
    """ClipWrapper (synthetic ViT-B/16, fp16) with clip.top_k = 3 and a view of it with top_k = 1: one set of weights"""
    from vilgod_amd.clip_wrapper import ClipWrapper
    from vilgod_amd.pipeline import default_preprocessor_cfg
    c3 = ClipWrapper(dict(default_preprocessor_cfg()['clip'], top_k=3), '/nonexistent', device=cuda, dtype='f16')
    c1 = c3.view()
    c1.top_k = 1
    assert c3.view().top_k == 3
    return c3, c1


def _im2col(crops):
    """[n,3,224,224] -> patch rows [pad256(n 196), 768]: row crop*196 + py*14 + px, column c*256 + i*16 + j (vg_vit_encode input_kind 2)"""
    n = crops.shape[0]
    p = crops.reshape(n, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(n * 196, 768)
    out = torch.zeros(((n * 196 + 255) // 256 * 256, 768), dtype=crops.dtype, device=crops.device)
    out[:n * 196] = p
    return out


def test_graph_classifier_selects_behind_the_replay(cuda, clips):
    from vilgod_amd.clip_wrapper import GraphClassifier
    c3, c1 = clips
    B = GraphClassifier.BUCKET
    g3 = GraphClassifier(c3.encoder.view(), c3.text_features, max_crops=2 * B, patch_width=768, top_k=3)
    g1 = GraphClassifier(c3.encoder.view(), c3.text_features, max_crops=2 * B, patch_width=768)
    assert g3.topk.shape == (2 * B, 3) and not hasattr(g1, 'topk')
    gen = torch.Generator().manual_seed(12)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for n in (B - 1, B, B + 1):
            crops = (torch.randn(n, 3, 224, 224, generator=gen) * 0.9).half().to(cuda)
            rows = _im2col(crops)
            want_p, want_top, want_score = c3.predict_probs(crops)
            p1, top1, score1 = c1.predict_probs(crops)
            assert want_top.shape == (n, 3) and top1.shape == (n,)
            for call in range(3):                                                    # plain, capture, replay
                for g in (g3, g1):
                    g.patch_buffer(n)[:len(rows)].copy_(rows)
                g3.topk.fill_(-7), g3.topk_score.fill_(-7.0)
                got = [t.clone() for t in g3.classify(n)]
                one = [t.clone() for t in g1.classify(n)]
                stream.synchronize()
                assert got[1].shape == (n, 3) and one[1].shape == (n,)
                assert torch.equal(got[1], want_top) and torch.equal(got[2].view(torch.int32), want_score.view(torch.int32)), (n, call)
                for a, b in ((got[0], one[0]), (got[0], want_p), (got[0], p1)):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (n, call)
                assert torch.equal(got[1][:, 0], one[1]) and torch.equal(got[2][:, 0].contiguous().view(torch.int32), one[2].view(torch.int32))
                assert torch.equal(one[1], top1) and torch.equal(one[2].view(torch.int32), score1.view(torch.int32))
                assert bool((g3.topk[n:] == -7).all()) and bool((g3.topk_score[n:] == -7.0).all())    # nothing behind the n rows
            want_idx, _ = R.order(got[0].cpu().numpy(), 3)
            assert np.array_equal(got[1].cpu().numpy(), want_idx)
    for g in (g3, g1):                                                                  # graphs were captured and replayed, two buckets at most
        assert 1 <= g.stats()['graphs_captured'] <= 2 and g.stats()['graph_launches'] >= 2, g.stats()


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
def _restate(pipe, table, k):
    """tests/clip_topk_ref.py's order + the reference's vote over the table read back -> per detection (detailed, names, scores, name, score)"""
    idx, score = R.order(table, k)
    V = 4 * k
    fine = np.array(pipe.class_list, dtype=object)[idx].reshape(-1, V)
    mapping = pipe.cfg['clip']['class_mapping']
    names = np.array([[mapping[c] for c in row] for row in fine], dtype=object)
    score = score.reshape(-1, V)
    voted = [R.reference_vote(names[c].astype(str), score[c]) for c in range(len(fine))]
    return fine, names, score, voted


def test_pipeline_with_top_k_3(cuda, clips):
    from vilgod_amd.frame_state import FrameState
    from vilgod_amd.pipeline import PseudoLabelPipeline, default_preprocessor_cfg
    c3, c1 = clips
    cfg3 = default_preprocessor_cfg()
    cfg3['clip'] = dict(cfg3['clip'], top_k=3)
    kw = dict(device=cuda, vit_dtype='f16', max_points=25_000, clip_model_path='/nonexistent', box_mode='fast', box_workers=0)
    p3 = PseudoLabelPipeline(cfg3, clip=c3, **kw)
    p1 = PseudoLabelPipeline(default_preprocessor_cfg(), clip=c1, **kw)
    pg = PseudoLabelPipeline(cfg3, clip=c3.view(), vit_graph=True, **kw)
    with pytest.raises(ValueError, match=r'clip\.top_k = 1 .* top_k = 3'):               # a wrapper built for another width
        PseudoLabelPipeline(default_preprocessor_cfg(), clip=c3, **kw)
    pts = synthetic.make_frame(3, 20_000, n_objects=12)
    poses = synthetic.make_poses(2, seed=4)
    fs3, res3 = p3.process_frame(pts, poses[1], poses[0], fnr=1)
    table = p3.last_probs.cpu().numpy()
    fs1, res1 = p1.process_frame(pts, poses[1], poses[0], fnr=1)
    assert np.array_equal(R.bits(table), R.bits(p1.last_probs.cpu().numpy()))
    rows = np.flatnonzero(fs3.valid)
    assert len(rows) >= 5 and np.array_equal(fs3.valid, fs1.valid) and table.shape == (4 * len(rows), len(p3.class_list))
    e3, e1 = fs3.cls[KEY], fs1.cls[KEY]
    for f in ('pred', 'detailed', 'score'):
        assert e3[f].shape == (fs3.n_detections, 12) and e1[f].shape == (fs1.n_detections, 4)
    # the first of each view's three is the top_k = 1 run's prediction for that view
    for f in ('pred', 'detailed'):
        assert np.array_equal(e3[f][rows][:, ::3], e1[f][rows])
    assert np.array_equal(R.bits(e3['score'][rows][:, ::3]), R.bits(e1['score'][rows]))
    fine, names, score, voted = _restate(p3, table, 3)
    assert np.array_equal(e3['detailed'][rows], fine) and np.array_equal(e3['pred'][rows], names)
    assert np.array_equal(R.bits(e3['score'][rows]), R.bits(score))
    for r, (name, s) in zip(rows, voted):
        assert str(e3['name'][r]) == name and R.bits(fs3.final_score(KEY, r)) == R.bits(s), (r, name, s)
    keep = [n in p3.class_names for n, _ in voted]
    assert list(res3['name']) == [n for (n, _), k in zip(voted, keep) if k]
    assert np.array_equal(R.bits(np.asarray(res3['score'], np.float32)), R.bits(np.array([s for (_, s), k in zip(voted, keep) if k], np.float32)))
    # a saved and loaded state keeps the width
    back = FrameState(1, poses[1], poses[0])
    back.sync(pickle.loads(pickle.dumps(fs3.serialize)))
    for f in ('pred', 'detailed', 'score'):
        assert back.cls[KEY][f].shape == (fs3.n_detections, 12)
    assert np.array_equal(back.cls[KEY]['detailed'][rows], e3['detailed'][rows]) and np.array_equal(R.bits(back.cls[KEY]['score'][rows]), R.bits(e3['score'][rows]))
    assert all(len(d['object_class_predictions'][KEY]) == 12 for d in fs3.serialize['_detections'] if d['valid'])
    # the captured loop on a worker stream: the same frame state
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for _ in range(2):                                                           # the handle's first call is plain, the second captures
            fsg, resg = pg.process_frame(pts, poses[1], poses[0], fnr=1)
        stream.synchronize()
    assert pg._graph_cls is not None and pg._graph_cls.top_k == 3 and pg._graph_cls.stats()['graph_launches'] >= 1
    eg = fsg.cls[KEY]
    assert np.array_equal(eg['detailed'], e3['detailed']) and np.array_equal(R.bits(eg['score']), R.bits(e3['score']))
    assert np.array_equal(eg['name'], e3['name']) and np.array_equal(eg['final'], e3['final'])
    # predict_clip_labels: the reference's flat order, crop-major and best first
    crops = (torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(1)) * 0.9).half().to(cuda)
    names_, scores_ = c3.predict_clip_labels(crops)
    probs, top, sc = c3.predict_probs(crops)
    assert len(names_) == len(scores_) == 15 and names_ == [p3.class_list[i] for i in top.cpu().numpy().reshape(-1)]
    assert np.array_equal(R.bits(np.array(scores_, np.float32)), R.bits(sc.cpu().numpy().reshape(-1)))
    assert len(c1.predict_clip_labels(crops)[0]) == 5


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_with_top_k_3(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess_data
    from test_cli import OVR, _load
    root = str(tmp_path / 'topk')
    preprocess_data.main(['preprocessor=waymo', f'dataset.DATA_PATH={root}', 'preprocessor.clip.top_k=3'] + OVR)
    out, idx, state = _load(root)
    assert len(out) == 6 and len(state) == 6
    classified = [d for st in state for d in st['_detections'] if KEY in d.get('object_class_predictions', {})]
    assert len(classified) >= 6
    for d in classified:
        assert len(d['object_class_predictions'][KEY]) == 12 and len(d['object_class_predictions_detailed'][KEY]) == 12
        assert d['object_class_predictions_score'][KEY].shape == (12,) and d['object_class_predictions_score'][KEY].dtype == np.float32
        s = d['object_class_predictions_score'][KEY].reshape(4, 3)
        assert np.all(s[:, :-1] >= s[:, 1:])                                          # a view's three, best first
    assert all(KEY in d['object_class'] for st in state for d in st['_detections'] if d['valid'])


# ---- capture -------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_equal_the_plain_launch(cuda):
    from vilgod_amd.clip_wrapper import clip_topk
    names, table = R.crafted_table(1203)
    n, k = len(table), 5
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        d = torch.from_numpy(table).to(cuda)
        want_top, want_score = [t.clone() for t in clip_topk(d, k)]
        top = torch.full((n + 1, k), -7, dtype=torch.int32, device=cuda)
        score = torch.full((n + 1, k), -7.0, dtype=torch.float32, device=cuda)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            clip_topk(d, k, top, score)
        for _ in range(2):
            top.fill_(-7), score.fill_(-7.0)
            graph.replay()
            stream.synchronize()
            assert torch.equal(top[:n], want_top) and torch.equal(score[:n].view(torch.int32), want_score.view(torch.int32))
            assert bool((top[n:] == -7).all()) and bool((score[n:] == -7.0).all())
    want_idx, _ = R.order(table, k)
    assert np.array_equal(want_top.cpu().numpy(), want_idx)
