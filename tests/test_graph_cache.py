"""The captured classification (clip_wrapper.GraphClassifier, include/vilgod_hip.h vg_vit_classify_graph / vg_graph_cache_*;
csrc/vit_graph.inc) where its claims were stated but unpinned:

  bucket padding   the crops that fill a bucket and every patch row behind them hold poison: classify(n) is the plain encode + scores of
                   the n clean crops on every bit, the persistent outputs behind the bucket keep a sentinel
  eviction         max_graphs = 2 over the crop counts 8, 16, 24, 8, 16, 24, 24, 8: the four counters follow independence_ref.LruModel
                   step by step, the results equal plain launches at every step; vg_graph_cache_limit refuses 0 and a null cache
  weights          vg_vit_set_weight (a GEMM weight behind a folded LayerNorm) and vg_vit_set_input_norm between replays: the next
                   classify equals a FRESH encoder's, differs from the old result, and the old graph is never replayed
  text             another text tensor = that text's scores (new key); text.copy_ in place = the new scores without a capture
  profiling        vg_vit_profile(1): plain launches, counters unchanged, results equal
  plan crossing    in a child process of its own (the kernels' launch attributes are set once per process): a handle's first call at 2
                   crops (folded fp32 stream), then 8 crops (fp16 pair, class-row last block) with 24 and with 100 classes (wide scores)
                   through the C ABI -- every call VG_OK and equal to plain launches of a second handle, a replay of each too

Every comparison is of bits.  The tower is a two-layer ViT-B/16 geometry in fp16 on a worker stream, fed patch rows of width 256
(single-channel levels, input_kind 3) and 768 (normalised channels, input_kind 2)."""
import ctypes
import functools
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import independence_ref as I
from vilgod_amd import clip_weights as cw

B16_2 = dict(cw.VIT_B16, layers=2)
FC0 = 'transformer.resblocks.0.mlp.c_fc.weight'
SEQUENCE = (8, 16, 24, 8, 16, 24, 24, 8)
OTHER_NORM = ((0.1, 0.5, 0.9), (0.2, 0.5, 1.5))
VG_OK, VG_ERR_ARG = 0, 1


# ------------------------------------------------------------------------------------------------------------------- CPU
def _run(model, keys):
    return [tuple(model.step(k).values()) for k in keys]          # (captured, launches, evicted, live)


def test_lru_model_on_hand_written_sequences():
    assert _run(I.LruModel(2), 'aaa') == [(0, 0, 0, 0), (1, 1, 0, 1), (1, 2, 0, 1)]                  # plain, capture, replay
    assert _run(I.LruModel(1), 'abab') == [(0, 0, 0, 0), (1, 1, 0, 1), (2, 2, 1, 1), (3, 3, 2, 1)]
    # b is touched before c arrives: a (not b) is the least recently used
    assert _run(I.LruModel(2), 'xabbca')[-2:] == [(3, 4, 1, 2), (4, 5, 2, 2)]
    assert _run(I.LruModel(2), 'xabac')[-1] == (3, 4, 1, 2) and I.LruModel(3).stats()['graphs_live'] == 0
    m = I.LruModel(2)
    assert _run(m, SEQUENCE) == [(0, 0, 0, 0), (1, 1, 0, 1), (2, 2, 0, 2), (3, 3, 1, 2), (4, 4, 2, 2), (5, 5, 3, 2), (5, 6, 3, 2), (6, 7, 4, 2)]
    assert m.live == [24, 8]
    # a replaced weight: one plain call, then a capture under the new key while the old graph still counts as live
    m = I.LruModel(4)
    _run(m, [(8, 0)] * 3)
    m.invalidate()
    assert _run(m, [(8, 1)] * 3) == [(1, 2, 0, 1), (2, 3, 0, 2), (2, 4, 0, 2)]


# ------------------------------------------------------------------------------------------------------------------- GPU plumbing
@functools.lru_cache(maxsize=None)
def _weights(seed=0):
    return cw.synthetic_vit_weights(seed, **B16_2)


def _rows(n):
    return (n * 196 + 255) // 256 * 256


def _patches(n, width, gen, device):
    """Clean patch rows of n crops [pad256(n 196), width], zeros behind the last crop, of the kind test_vit's captured test uses."""
    p = torch.zeros(_rows(n), width, dtype=torch.float16)
    if width == 768:
        p[:n * 196] = (torch.randn(n * 196, 768, generator=gen) * 0.8).half()
    else:
        p[:n * 196] = (torch.randint(0, 256, (n * 196, 256), generator=gen).float() / 256.0).half()
    return p.to(device)


def _encoder(cuda, weights=None, norm=None):
    from vilgod_amd._lib import lib, check
    from vilgod_amd.clip_wrapper import VitEncoder
    enc = VitEncoder(weights or _weights(), dtype='f16', device=cuda)
    if norm is not None:
        check(lib.vg_vit_set_input_norm(enc._h, (ctypes.c_float * 3)(*norm[0]), (ctypes.c_float * 3)(*norm[1])), 'vg_vit_set_input_norm')
    return enc


def _plain(enc, p, n, text):
    from vilgod_amd.clip_wrapper import clip_scores
    return clip_scores(enc.encode_patches(p, n), text)


def _same(got, want, what):
    for g, w, name in zip(got, want, ('probs', 'top1', 'score')):
        assert torch.equal(I.bits(g), I.bits(w)), f'{what}: {name} differs from the plain launches'


def _classify(g, n):
    return [t.clone() for t in g.classify(n)]


# ------------------------------------------------------------------------------------------------------------------- bucket padding
@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_bucket_padding_is_never_read_into_a_result(cuda, width):
    """n = 5 and 13 crops in buckets of 8 and 16: the patch rows of crops n .. nb - 1 and every row behind them (to the end of the
    24-crop buffer) hold NaN, +-Inf or 65504; classify(n) -- as the handle's plain first call, as a capture and as a replay -- equals
    clip_scores(encode_patches(clean, n)); rows nb .. of feat, probs, top1 and score keep their sentinel."""
    from vilgod_amd.clip_wrapper import GraphClassifier
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    enc = _encoder(cuda)
    plain = enc.view()
    g = GraphClassifier(enc, text, max_crops=24, patch_width=width)
    gen = torch.Generator().manual_seed(width)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for n, nb in ((5, 8), (13, 16)):
            p = _patches(n, width, gen, cuda)
            want = _plain(plain, p, n, text)
            for kind in I.POISONS:
                for call in range(3):
                    buf = g.patch_buffer(n)
                    buf.copy_(I.poison_row(width, torch.float16, kind, cuda)[None, :].expand_as(buf))
                    buf[:n * 196].copy_(p[:n * 196])
                    g.feat.fill_(-7.0), g.probs.fill_(-7.0), g.top1.fill_(-7), g.score.fill_(-7.0)
                    got = _classify(g, n)
                    stream.synchronize()
                    assert all(bool(torch.isfinite(t.float()).all()) for t in got)
                    _same(got, want, f'{n} crops, {kind}, call {call}')
                    for t in (g.feat, g.probs, g.top1, g.score):
                        assert bool((t[nb:] == -7).all()) and t[nb:].numel() > 0, f'{n} crops, {kind}: rows behind the bucket were written'
                        assert not bool((t[:n] == -7).any())
    st = g.stats()
    assert st['graphs_captured'] == 2 and st['graph_launches'] == 17, st           # 18 calls, the handle's first one plain


# ------------------------------------------------------------------------------------------------------------------- eviction
@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_eviction_follows_the_lru_model(cuda, width):
    from vilgod_amd._lib import lib
    from vilgod_amd.clip_wrapper import GraphClassifier
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    enc = _encoder(cuda)
    plain = enc.view()
    g = GraphClassifier(enc, text, max_crops=24, max_graphs=2, patch_width=width)
    assert lib.vg_graph_cache_limit(g._cache, 0) == VG_ERR_ARG and lib.vg_graph_cache_limit(g._cache, -1) == VG_ERR_ARG
    assert lib.vg_graph_cache_limit(None, 2) == VG_ERR_ARG
    model = I.LruModel(2)
    gen = torch.Generator().manual_seed(7 + width)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        for step, n in enumerate(SEQUENCE):
            p = _patches(n, width, gen, cuda)
            g.patch_buffer(n)[:_rows(n)].copy_(p)
            got = _classify(g, n)
            want = _plain(plain, p, n, text)
            stream.synchronize()
            _same(got, want, f'step {step}, {n} crops')
            assert g.stats() == model.step(n), (step, n, g.stats(), model.stats())
    assert g.stats() == {'graphs_captured': 6, 'graph_launches': 7, 'graphs_evicted': 4, 'graphs_live': 2}


# ------------------------------------------------------------------------------------------------------------------- weights, norm
def _set_weight(enc, name, t):
    from vilgod_amd._lib import lib, check
    t = t.detach().float().contiguous().cpu()
    with torch.cuda.device(enc.device):
        check(lib.vg_vit_set_weight(enc._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), 'vg_vit_set_weight')


@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_replaced_weights_are_never_replayed(cuda, width):
    """After a capture and replays: block 0's c_fc weight (it feeds the fold of ln_2) is replaced through vg_vit_set_weight, and at width
    256 the input normalisation through vg_vit_set_input_norm.  Each change invalidates the handle's derived tensors, so the next call
    runs as plain launches (they are rebuilt outside any capture: no counter moves) and the one after captures under the new weight
    generation, the old graph staying in the cache unused.  Every result equals a fresh encoder built with the new values."""
    from vilgod_amd.clip_wrapper import GraphClassifier
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    n = 8
    p = _patches(n, width, torch.Generator().manual_seed(3), cuda)
    enc = _encoder(cuda)
    g = GraphClassifier(enc, text, max_crops=8, patch_width=width)
    model = I.LruModel(32)
    stream = torch.cuda.Stream(device=cuda)
    changes = [('weight', None)] + ([('norm', OTHER_NORM)] if width == 256 else [])
    wd, norm, gen = dict(_weights()), None, 0
    with torch.cuda.stream(stream):
        g.patch_buffer(n)[:_rows(n)].copy_(p)
        old = None
        for what, value in [(None, None)] + changes:
            if what == 'weight':
                wd[FC0] = wd[FC0].flip(0) * 1.25
                _set_weight(enc, FC0, wd[FC0])
            elif what == 'norm':
                from vilgod_amd._lib import lib
                norm = value
                assert lib.vg_vit_set_input_norm(enc._h, (ctypes.c_float * 3)(*norm[0]), (ctypes.c_float * 3)(*norm[1])) == VG_OK
            if what:
                gen += 1
                model.invalidate()
            want = _plain(_encoder(cuda, wd, norm), p, n, text)
            stream.synchronize()
            for call in range(3):                       # plain, capture, replay
                got = _classify(g, n)
                stream.synchronize()
                _same(got, want, f'after {what}, call {call}')
                assert g.stats() == model.step((n, gen)), (what, call, g.stats(), model.stats())
            if old is not None:
                assert not torch.equal(I.bits(old[0]), I.bits(got[0])), f'{what}: the result did not change'
            old = got
    assert g.stats()['graphs_captured'] == 1 + len(changes) == g.stats()['graphs_live']


# ------------------------------------------------------------------------------------------------------------------- text
@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_text_is_keyed_by_pointer_and_read_at_replay(cuda, width):
    from vilgod_amd.clip_wrapper import GraphClassifier
    text_a = cw.synthetic_text_features(0, 24, 512).to(cuda)
    text_b = cw.synthetic_text_features(1, 24, 512).to(cuda)
    text_c = cw.synthetic_text_features(2, 24, 512).to(cuda)
    n = 8
    p = _patches(n, width, torch.Generator().manual_seed(4), cuda)
    enc = _encoder(cuda)
    plain = enc.view()
    g = GraphClassifier(enc, text_a, max_crops=8, patch_width=width)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        g.patch_buffer(n)[:_rows(n)].copy_(p)
        wants = [_plain(plain, p, n, t) for t in (text_a, text_b, text_c)]
        stream.synchronize()
        assert not torch.equal(wants[0][0], wants[1][0]) and not torch.equal(wants[1][0], wants[2][0])
        for _ in range(2):
            got = _classify(g, n)
        stream.synchronize()
        _same(got, wants[0], 'text a')
        assert g.stats()['graphs_captured'] == 1
        got = [t.clone() for t in g.classify(n, text_b)]              # another tensor of the same shape: a new key
        stream.synchronize()
        _same(got, wants[1], 'text b')
        assert g.stats()['graphs_captured'] == 2 and g.stats()['graph_launches'] == 2
        text_b.copy_(text_c)                                          # in place: the same key, the node reads the new values
        got = _classify(g, n)
        stream.synchronize()
        _same(got, wants[2], 'text c copied into b')
        assert g.stats()['graphs_captured'] == 2 and g.stats()['graph_launches'] == 3


# ------------------------------------------------------------------------------------------------------------------- profiling
@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_profiling_runs_plain_launches(cuda, width):
    from vilgod_amd.clip_wrapper import GraphClassifier
    text = cw.synthetic_text_features(0, 24, 512).to(cuda)
    n = 8
    p = _patches(n, width, torch.Generator().manual_seed(5), cuda)
    enc = _encoder(cuda)
    g = GraphClassifier(enc, text, max_crops=8, patch_width=width)
    stream = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(stream):
        g.patch_buffer(n)[:_rows(n)].copy_(p)
        for _ in range(3):
            want = _classify(g, n)
        stream.synchronize()
        before = g.stats()
        assert before['graphs_captured'] == 1 and before['graph_launches'] == 2
        enc.profile(True)
        try:
            g.probs.fill_(-7.0)
            got = _classify(g, n)
            stream.synchronize()
            launches, _, _ = enc.profile_read()
        finally:
            enc.profile(False)
        assert launches > 0                                           # the profiled call really launched GEMMs one by one
        _same(got, want, 'profiled')
        assert g.stats() == before
        got = _classify(g, n)                                         # and the graph is still there
        stream.synchronize()
        _same(got, want, 'after profiling')
        assert g.stats() == dict(before, graph_launches=3)


# ------------------------------------------------------------------------------------------------------------------- plan crossing
CHILD = '''
import ctypes, sys
import torch
sys.path.insert(0, {root!r})
import independence_ref as I
from vilgod_amd import clip_weights as cw
from vilgod_amd._lib import lib, ptr, stream_ptr
from vilgod_amd.clip_wrapper import VitEncoder

dev = torch.device('cuda:0')
cfg = dict(cw.VIT_B16, layers=2)
assert I.plan(cfg, 2) == ('fold', False) and I.plan(cfg, 8) == ('pair', True)
wd = cw.synthetic_vit_weights(0, **cfg)
graph, plain = VitEncoder(wd, dtype='f16', device=dev), VitEncoder(wd, dtype='f16', device=dev)
cache = ctypes.c_void_p()
assert lib.vg_graph_cache_create(ctypes.byref(cache)) == 0
texts = {{k: cw.synthetic_text_features(6, k, 512).to(dev) for k in (24, 100)}}
rows = (8 * 196 + 255) // 256 * 256
width = {width}
gen = torch.Generator().manual_seed(11)
if width == 768:
    patches = (torch.randn(rows, 768, generator=gen) * 0.8).half().to(dev)
else:
    patches = (torch.randint(0, 256, (rows, 256), generator=gen).float() / 256.0).half().to(dev)
kind = 2 if width == 768 else 3
ws = [torch.zeros(int(lib.vg_vit_workspace_bytes(e._h, 8)), dtype=torch.uint8, device=dev) for e in (graph, plain)]
assert ws[0].numel() == I.workspace_bytes(cfg, 8)


def outputs(k):
    return [torch.full((8, 512), -7.0, device=dev), torch.full((8, k), -7.0, device=dev), torch.full((8,), -7, dtype=torch.int32, device=dev),
            torch.full((8,), -7.0, device=dev)]


out = {{k: outputs(k) for k in (24, 100)}}           # persistent: their pointers are part of the key
stream = torch.cuda.Stream(device=dev)
with torch.cuda.stream(stream):
    for step, (n, k) in enumerate([(2, 24), (8, 24), (8, 100), (8, 24), (8, 100), (2, 24), (8, 24), (8, 100), (2, 24)]):
        feat, probs, top1, score = out[k]
        for t in out[k]:
            t.fill_(-7)
        rc = lib.vg_vit_classify_graph(graph._h, cache, ptr(patches), kind, n, ptr(ws[0]), ptr(feat), ptr(texts[k]), 512, k, ptr(probs), ptr(top1),
                                       ptr(score), stream_ptr())
        stream.synchronize()
        assert rc == 0, (step, n, k, rc)
        got = [t[:n].clone() for t in (probs, top1, score)]
        w = outputs(k)
        assert lib.vg_vit_encode(plain._h, ptr(patches), kind, n, ptr(ws[1]), ptr(w[0]), stream_ptr()) == 0
        fn = lib.vg_clip_scores if k <= 64 else lib.vg_clip_scores_wide
        assert fn(ptr(w[0]), n, 512, ptr(texts[k]), k, ptr(w[1]), ptr(w[2]), ptr(w[3]), stream_ptr()) == 0
        stream.synchronize()
        for g, t in zip(got, w[1:]):
            assert torch.isfinite(g.float()).all() and torch.equal(I.bits(g), I.bits(t[:n])), (step, n, k)
c, r, e, l = (ctypes.c_int64(0) for _ in range(4))
assert lib.vg_graph_cache_stats2(cache, ctypes.byref(c), ctypes.byref(r), ctypes.byref(e), ctypes.byref(l)) == 0
# three launch forms, the first call of each plain: six of the nine calls go through a graph, three graphs
assert (c.value, r.value, e.value, l.value) == (3, 6, 0, 3), (c.value, r.value, e.value, l.value)
lib.vg_graph_cache_destroy(cache)
print('PLAN-CROSSING-OK')
'''


@pytest.mark.gpu
@pytest.mark.parametrize('width', [256, 768])
def test_capture_after_a_plan_crossing(cuda, width, tmp_path):
    """The kernels' dynamic-LDS attributes are set lazily, once per kernel instantiation and process, and must not be set inside a
    capture.  A handle whose first call came at 2 crops (ViT-B/16 geometry: folded fp32 stream, full last block) has never launched
    the pair-stream epilogue or the class-row kernels when 8 crops arrive, nor the wide scores kernel when 100 classes do.  In a
    process of its own, where no earlier test has set anything: the calls 2 / 24, 8 / 24, 8 / 100 (crops / classes), a replay of each
    and a third round all return VG_OK and equal plain launches on a second handle; every launch form's first call ran plain (3
    graphs, 6 graph launches of 9 calls).  The child runs once, with its own time limit."""
    script = tmp_path / 'plan_crossing.py'
    script.write_text(textwrap.dedent(CHILD).format(root=os.path.dirname(os.path.abspath(__file__)), width=width))
    env = {k: v for k, v in os.environ.items() if not k.startswith('VG_')}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=240, env=env, cwd=root)
    assert res.returncode == 0 and 'PLAN-CROSSING-OK' in res.stdout, f'exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}'
