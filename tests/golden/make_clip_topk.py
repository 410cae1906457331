"""Generates tests/golden/clip_topk_golden.npz by running the REFERENCE's own Python (stub-imported, see oracle/refstubs.py) on
seeded inputs.  Run only where the reference tree is present:

    python tests/golden/make_clip_topk.py

  * ClipWrapper.predict_clip_labels (src/utils/clip_utils.py:34-63) runs unbound on a stand-in `self` whose `model.encode_image`
    hands out seeded unit features: the method's own normalisation, softmax, argpartition and argsort produce the names and scores,
    for clip.top_k = 1, 2, 3, 5, 16 and class lists of 24 and 100 names, 40 detections x 4 views each.
  * The names are mapped and reshaped as zero_shot_detector.py:412-415 does, and LidarFrame.update_object_classes
    (src/vilgod/lidar_frame.py:260-291) runs unbound on stand-in detections: the voted name and float32 score.
  * `vote_*`: 4 000 seeded rows at 4 and at 7 entries per row, and what `frame_state.vote` of the commit BEFORE the top-k work
    (PARENT below) returns for them -- the bits the extended vote must keep returning below 8 entries.

The fixture is data (inputs + the reference's outputs); no reference source is stored.  The generator asserts what the tests rely on:
no row has two equal probabilities among its k + 1 largest (the reference's order among equal scores is implementation-defined),
and for every k >= 3 some detection has a name with 8 or more entries (numpy's pairwise float32 sum)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import refstubs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PARENT = 'fedac2b'
KS = (1, 2, 3, 5, 16)
N_DET, N_VIEWS, DIM = 40, 4, 512
MAPPED = ('Background', 'Cyclist', 'Pedestrian', 'Vehicle')


def unit(rng, n, d):
    x = rng.normal(size=(n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)


def class_tables(K):
    fine = [f'class{i:03d}' for i in range(K)]
    rng = np.random.default_rng(77 + K)
    # (half of the fine classes map to one name, as the shipped lists do for Background: names with many entries per detection)
    mapping = {c: MAPPED[int(m)] for c, m in zip(fine, rng.choice(len(MAPPED), size=K, p=(0.5, 0.1, 0.15, 0.25)))}
    return fine, mapping


def run_reference(K, k, feat, text):
    from src.utils.clip_utils import ClipWrapper
    from src.vilgod.lidar_frame import LidarFrame
    fine, mapping = class_tables(K)
    F, T = torch.from_numpy(feat), torch.from_numpy(text)
    model = types.SimpleNamespace(encode_image=lambda split: F[split[:, 0]].clone())
    self_ = types.SimpleNamespace(device='cpu', top_k=k, split_size=50, model=model, text_features=T,
                                  preprocess=lambda i: torch.tensor([i]), id_to_class_dict=dict(enumerate(fine)))
    n = len(feat)
    detailed, scores = ClipWrapper.predict_clip_labels(self_, list(range(n)))
    # the table the method formed (clip_utils.py:41-47: the same statements on the same splits; checked against its scores below)
    table = []
    for split in torch.split(torch.arange(n), 50):
        f = F[split].clone()
        f /= f.norm(dim=-1, keepdim=True)
        table.append((100.0 * f @ T.T).softmax(dim=-1))
    table = torch.cat(table, dim=0).numpy()
    idx = np.array([fine.index(c) for c in detailed]).reshape(n, k)
    got = np.array(scores, np.float32).reshape(n, k)
    assert np.array_equal(table[np.arange(n)[:, None], idx].view(np.uint32), got.view(np.uint32)), 'the restated table is not the method\'s'
    top = -np.sort(-table, axis=1)[:, :min(K, k + 1)]
    assert np.all(np.diff(top, axis=1) < 0), f'K={K} k={k}: equal probabilities among the k + 1 largest'
    # zero_shot_detector.py:412-415
    length = N_DET
    names = np.stack([mapping[c] for c in detailed]).reshape((length, -1))
    detailed_a = np.stack(detailed).reshape(length, -1)
    score_a = np.stack(scores).reshape(length, -1)
    assert score_a.dtype == np.float32

    class Det:
        def __init__(self):
            self.e = {}

        def add_object_entry(self, what, key, value):
            self.e[what] = value
    frame = types.SimpleNamespace(detections=[Det() for _ in range(length)])
    LidarFrame.update_object_classes(frame, names, detailed_a, score_a, [True] * length, key='clip', aggregation='voting')
    voted = np.array([d.e['object_class'] for d in frame.detections])
    voted_score = np.array([d.e['object_class_score'] for d in frame.detections])
    assert voted_score.dtype == np.float32, voted_score.dtype
    most = max(int(np.unique(r, return_counts=True)[1].max()) for r in names)
    if k >= 3:
        assert most >= 8, f'K={K} k={k}: no name with 8 or more entries'
    return dict(table=table, idx=idx.astype(np.int32), detailed=detailed_a, names=names, scores=score_a, voted=voted, voted_score=voted_score), most


def parent_vote():
    src = subprocess.run(['git', 'show', f'{PARENT}:vilgod_amd/frame_state.py'], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    start = src.index('def vote(')
    ns = {'np': np}
    exec(src[start:src.index('\ndef ', start + 1)], ns)
    return ns['vote']


def main():
    refstubs.install()
    sys.modules.setdefault('clip', types.ModuleType('clip'))
    store = {'ks': np.array(KS), 'mapped': np.array(MAPPED)}
    for K in (24, 100):
        rng = np.random.default_rng(20260000 + K)
        feat = unit(rng, N_DET * N_VIEWS, DIM) * np.float32(1.7)          # not unit: the method normalises them itself
        text = unit(rng, K, DIM)
        fine, mapping = class_tables(K)
        store[f'fine_{K}'] = np.array(fine)
        store[f'mapping_{K}'] = np.array([mapping[c] for c in fine])
        for k in KS:
            r, most = run_reference(K, k, feat, text)
            if k == KS[0]:
                store[f'table_{K}'] = r['table']
            else:
                assert np.array_equal(store[f'table_{K}'].view(np.uint32), r['table'].view(np.uint32))
            for key in ('idx', 'detailed', 'names', 'scores', 'voted', 'voted_score'):
                store[f'{key}_{K}_{k}'] = r[key]
            print(f'K={K} k={k}: largest count of one name in a detection {most}')
    vote = parent_vote()
    for width in (4, 7):
        rng = np.random.default_rng(4000 + width)
        ids = rng.integers(0, len(MAPPED), size=(4000, width))
        sc = rng.uniform(0.01, 0.99, size=(4000, width)).astype(np.float32)
        sc[::5] = np.round(sc[::5], 1)                                    # coarse scores: equal means meet the `>` scan
        win, score = vote(ids, sc, sorted(MAPPED))
        assert score.dtype == np.float32
        store[f'vote_ids_{width}'], store[f'vote_scores_{width}'] = ids.astype(np.int8), sc
        store[f'vote_win_{width}'], store[f'vote_final_{width}'] = win.astype(np.int8), score
    np.savez_compressed(os.path.join(OUT, 'clip_topk_golden.npz'), **store)
    print('clip_topk_golden.npz', os.path.getsize(os.path.join(OUT, 'clip_topk_golden.npz')), 'bytes')


if __name__ == '__main__':
    main()
