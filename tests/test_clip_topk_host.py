"""Top-k class selection (csrc/clip_topk.hip, csrc/clip_topk_key.inc) through vg_clip_topk_host, which orders rows under the
comparator the kernel runs: indices and score BITS equal to the numpy order of tests/clip_topk_ref.py on crafted tables (ties at the
lane and stride seams, a tie group the cut goes through, zeros, denormals, signed zeros, NaNs), the refusals, the reference's own
predict_clip_labels + update_object_classes results (tests/golden/clip_topk_golden.npz) through vote_classes and
FrameState.detection_dict, the vote's unchanged bits below 8 entries, and clip.top_k's argument handling.  No GPU."""
import os
import types

import numpy as np
import pytest

import clip_topk_ref as R
from vilgod_amd import build
from vilgod_amd._lib import lib
from vilgod_amd.clip_wrapper import MAX_TOPK, validate_top_k
from vilgod_amd.frame_state import FrameState, vote

KEY = 'clip_a_point_representation_of_a'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'clip_topk_golden.npz'))


def _equal(idx, score, want_idx, want_score, label):
    assert np.array_equal(idx, want_idx), (label, np.argwhere(idx != want_idx)[:5])
    assert np.array_equal(R.bits(score), R.bits(want_score)), (label, np.argwhere(R.bits(score) != R.bits(want_score))[:5])


# ---- build ---------------------------------------------------------------------------------------------------------------------------
def test_build_lists_the_source_and_the_kernel_has_no_scratch():
    assert build.SOURCES['clip_topk.hip'] == ['-ffp-contract=off']
    assert build.check_scratch('clip_topk.hip', '') == []
    assert MAX_TOPK == R.MAX_TOPK == 32
    assert validate_top_k(32) == 32 and validate_top_k(np.int32(5), 5) == 5


# ---- the order -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', R.SIZES_K)
def test_host_equals_the_numpy_order_on_crafted_tables(K):
    names, table = R.crafted_table(K)
    for k in R.ks_for(K):
        want_idx, want_score = R.order(table, k)
        st, idx, score = R.host(lib, table, k)
        assert st == 0
        _equal(idx[:-1], score[:-1], want_idx, want_score, (K, k, names))
        assert np.all(idx[-1] == R.SENTINEL_I) and np.all(score[-1] == R.SENTINEL_F)        # nothing behind the last row
        for n in (0, 1, 3):
            st, idx, score = R.host(lib, table[2:2 + n], k)
            assert st == 0
            _equal(idx[:n], score[:n], want_idx[2:2 + n], want_score[2:2 + n], (K, k, n))
            assert np.all(idx[n:] == R.SENTINEL_I) and np.all(score[n:] == R.SENTINEL_F)


def test_the_crafted_rows_hold_what_they_are_named_for():
    """The patterns are there at the sizes that have room for them, and the numpy order treats them as the contract says."""
    rows = R.crafted(257)
    idx, score = R.order(np.stack([rows['one_stride'], rows['neighbours'], rows['seam_63_64_65']]), 5)
    assert list(idx[0, :3]) == [5, 69, 133] and list(idx[1, :3]) == [5, 6, 7] and list(idx[2, :3]) == [63, 64, 65]
    assert np.all(score[:, :3] == np.float32(0.75)) and np.all(score[:, 3:] < np.float32(0.75))
    cut = rows['cut_group']
    assert np.sum(cut == np.float32(0.75)) == 9                                   # k = 2 and k = 5 cut through the nine
    idx, score = R.order(cut[None], 5)
    assert list(idx[0]) == list(np.flatnonzero(cut == np.float32(0.75))[:5])
    idx, score = R.order(rows['all_equal'][None], 32)
    assert list(idx[0]) == list(range(32))
    idx, score = R.order(rows['signed_zeros'][None], 5)
    assert list(idx[0]) == [0, 1, 2, 3, 4] and list(np.signbit(score[0])) == [True, False, True, False, True]
    idx, score = R.order(rows['zeros_denormals'][None], 5)
    z = rows['zeros_denormals']
    assert np.sum((z > 0) & (z < np.finfo(np.float32).tiny)) == 4 and np.all(z[idx[0, :4]] > 0) and z[idx[0, 4]] == 0 and idx[0, 4] == np.flatnonzero(z == 0)[0]
    idx, score = R.order(rows['all_nan'][None], 5)
    assert list(idx[0]) == [0, 1, 2, 3, 4] and np.isnan(score).all()
    one = rows['one_nan']
    idx, score = R.order(one[None], 257)
    assert idx[0, -1] == np.flatnonzero(np.isnan(one))[0] and not np.isnan(score[0, :-1]).any()
    m = rows['mostly_nan']
    idx, score = R.order(m[None], 5)
    assert list(score[0, :3]) == [0.5, 0.5, -np.inf] and idx[0, 0] < idx[0, 1] and list(idx[0, 3:]) == list(np.flatnonzero(np.isnan(m))[:2])


def test_a_nan_is_written_as_it_stands():
    table = np.zeros((1, 70), np.float32)
    table.view(np.uint32)[0, :] = 0x7fc00000
    table.view(np.uint32)[0, 3] = 0xffc12345                                       # a payload and a sign
    table.view(np.uint32)[0, 66] = 0x7f800001                                       # a signalling pattern
    st, idx, score = R.host(lib, table, 5)
    assert st == 0 and list(idx[0]) == [0, 1, 2, 3, 4]
    assert R.bits(score[0])[3] == 0xffc12345
    st, idx, score = R.host(lib, table, 32)
    assert list(idx[0]) == list(range(32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['k0', 'k_negative', 'k33', 'k_above_classes', 'no_classes', 'negative_classes', 'null_probs', 'null_idx',
                                  'null_score'])
def test_refusals_leave_the_outputs_untouched(case):
    table = R.crafted_table(64)[1][:3]
    kw = {'k0': dict(k=0), 'k_negative': dict(k=-1), 'k33': dict(k=33), 'k_above_classes': dict(k=5, n_classes=4),
          'no_classes': dict(k=1, n_classes=0), 'negative_classes': dict(k=1, n_classes=-3), 'null_probs': dict(k=2, null=('probs',)),
          'null_idx': dict(k=2, null=('idx',)), 'null_score': dict(k=2, null=('score',))}[case]
    st, idx, score = R.host(lib, table, **kw)
    assert st == 1                                                                  # VG_ERR_ARG
    assert np.all(idx == R.SENTINEL_I) and np.all(score == R.SENTINEL_F)


def test_no_rows_is_ok_and_writes_nothing():
    table = R.crafted_table(64)[1]
    for n in (0, -2):
        st, idx, score = R.host(lib, table, 3, n=n)
        assert st == 0 and np.all(idx == R.SENTINEL_I) and np.all(score == R.SENTINEL_F)
    st, idx, score = R.host(lib, table, 3, n=0, null=('probs', 'idx', 'score'))     # null pointers matter only with rows
    assert st == 0
    assert R.host(lib, table, 33, n=0)[0] == 1                                      # the arguments are checked first


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _vote_through_the_pipeline(g, K, k, idx, score):
    """vote_classes (unbound: it reads the class tables and the widths only) + FrameState -> the frame state"""
    from vilgod_amd.pipeline import PseudoLabelPipeline
    fine = [str(c) for c in g[f'fine_{K}']]
    cfg = dict(name='clip', prompt_template='a point representation of a {}', class_list=fine, top_k=k,
               class_mapping={c: str(m) for c, m in zip(fine, g[f'mapping_{K}'])})
    self_ = types.SimpleNamespace(projection=types.SimpleNamespace(num_views=4))
    PseudoLabelPipeline._init_classes(self_, cfg)
    assert self_.cls_key == KEY and self_.top_k == k
    C = len(idx) // 4
    fs = FrameState(0, np.eye(4), np.eye(4))
    fs.set_clusters(np.arange(C, dtype=np.int64), np.arange(C, dtype=np.int32), np.arange(C + 1, dtype=np.int32))
    PseudoLabelPipeline.vote_classes(self_, fs, self_.cls_key, np.ones(C, bool), idx, score)
    return fs


@pytest.mark.parametrize('K', [24, 100])
def test_host_selection_vote_and_detection_dict_equal_the_reference(golden, K):
    table = golden[f'table_{K}']
    fine = golden[f'fine_{K}']
    for k in golden['ks']:
        k = int(k)
        st, idx, score = R.host(lib, table, k)
        assert st == 0
        idx, score = idx[:-1], score[:-1]
        C = len(table) // 4
        assert np.array_equal(idx, golden[f'idx_{K}_{k}']), (K, k)                     # no row left out: the generator found no tie
        assert np.array_equal(fine[idx].reshape(C, -1), golden[f'detailed_{K}_{k}'])
        assert np.array_equal(R.bits(score.reshape(C, -1)), R.bits(golden[f'scores_{K}_{k}']))
        fs = _vote_through_the_pipeline(golden, K, k, idx, score)
        names = golden[f'names_{K}_{k}']
        most = 0
        for c in range(C):
            d = fs.detection_dict(c)
            assert d['object_class_predictions'][KEY].shape == (4 * k,)
            assert np.array_equal(d['object_class_predictions'][KEY], names[c])
            assert np.array_equal(d['object_class_predictions_detailed'][KEY], golden[f'detailed_{K}_{k}'][c])
            assert np.array_equal(R.bits(d['object_class_predictions_score'][KEY]), R.bits(golden[f'scores_{K}_{k}'][c]))
            assert d['object_class'][KEY] == golden[f'voted_{K}_{k}'][c], (K, k, c)
            s = d['object_class_score'][KEY]
            assert isinstance(s, np.float32) and R.bits(s) == R.bits(golden[f'voted_score_{K}_{k}'][c]), (K, k, c, s)
            most = max(most, int(np.unique(names[c], return_counts=True)[1].max()))
            assert R.reference_vote(names[c], golden[f'scores_{K}_{k}'][c])[0] == golden[f'voted_{K}_{k}'][c]      # the restatement the GPU tests use
            assert R.bits(R.reference_vote(names[c], golden[f'scores_{K}_{k}'][c])[1]) == R.bits(golden[f'voted_score_{K}_{k}'][c])
        if k >= 3:
            assert most >= 8                                                           # numpy's pairwise sum took part


def test_the_width_survives_a_round_trip_of_the_frame_state(golden):
    K, k = 24, 3
    st, idx, score = R.host(lib, golden[f'table_{K}'], k)
    fs = _vote_through_the_pipeline(golden, K, k, idx[:-1], score[:-1])
    fs.valid[::3] = False
    data = fs.serialize
    back = FrameState(0, np.eye(4), np.eye(4))
    back.sync(data)
    again = FrameState.from_compact(fs.compact())
    for other in (back, again):
        for f in ('pred', 'detailed', 'score'):
            assert other.cls[KEY][f].shape == (fs.n_detections, 4 * k)
        for c in range(fs.n_detections):
            a, b = fs.detection_dict(c), other.detection_dict(c)
            for f in ('object_class_predictions', 'object_class_predictions_detailed', 'object_class_predictions_score'):
                assert np.array_equal(a[f][KEY], b[f][KEY])
            assert a['object_class'][KEY] == b['object_class'][KEY] and R.bits(a['object_class_score'][KEY]) == R.bits(b['object_class_score'][KEY])


# ---- the vote below 8 entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [4, 7])
def test_vote_keeps_its_bits_below_eight_entries(golden, width):
    ids, sc = golden[f'vote_ids_{width}'].astype(np.int64), golden[f'vote_scores_{width}']
    assert ids.shape == (4000, width)
    win, final = vote(ids, sc, sorted(str(m) for m in golden['mapped']))
    assert final.dtype == np.float32
    assert np.array_equal(win, golden[f'vote_win_{width}'].astype(np.int64))
    assert np.array_equal(R.bits(final), R.bits(golden[f'vote_final_{width}']))


def test_vote_is_numpys_mean_from_eight_entries_on():
    """The extended vote against the restated reference rule on seeded rows where names have 8 and more entries (4 x 3, 4 x 5, 6 x 5,
    4 x 16), and the sequential sum it replaces does differ there."""
    mapped = ['Background', 'Cyclist', 'Pedestrian', 'Vehicle']
    differs = 0
    for width in (12, 20, 30, 64):
        rng = np.random.default_rng(width)
        ids = rng.integers(0, 4, size=(1000, width))
        sc = rng.uniform(0.0, 1.0, size=(1000, width)).astype(np.float32)
        win, final = vote(ids, sc, mapped)
        for c in range(len(ids)):
            name, s = R.reference_vote(np.array(mapped)[ids[c]], sc[c])
            assert mapped[win[c]] == name and R.bits(final[c]) == R.bits(s), (width, c)
            seq = np.float32(0)
            for v in sc[c][ids[c] == win[c]]:
                seq = seq + v
            differs += R.bits(np.float32(seq / np.float32(np.sum(ids[c] == win[c])))) != R.bits(s)
    assert differs > 0


# ---- clip.top_k ----------------------------------------------------------------------------------------------------------------------
def _clip_cfg(top_k, n_classes=6):
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = dict(default_preprocessor_cfg()['clip'])
    cfg['class_list'] = list(cfg['class_list'])[:n_classes]
    cfg['top_k'] = top_k
    return cfg


@pytest.fixture()
def no_tower(monkeypatch):
    """ClipWrapper without a device: the tower's weights and the encoder are stand-ins (the argument handling runs in front of both)."""
    import torch
    from vilgod_amd import clip_weights, clip_wrapper
    monkeypatch.setattr(clip_weights, 'synthetic_vit_weights', lambda seed, **kw: {'proj': torch.zeros(8, 4)})
    monkeypatch.setattr(clip_wrapper, 'VitEncoder', lambda weights, dtype, device: types.SimpleNamespace(view=lambda: 'view'))
    return clip_wrapper.ClipWrapper


@pytest.mark.parametrize('top_k', [1, 2, 3, 6, np.int64(4)])
def test_clipwrapper_accepts_top_k(no_tower, top_k):
    clip = no_tower(_clip_cfg(top_k), '/nonexistent', device='cpu')
    assert clip.top_k == int(top_k) and type(clip.top_k) is int
    assert clip.view().top_k == int(top_k)


def test_clipwrapper_accepts_the_largest_top_k(no_tower):
    from vilgod_amd.pipeline import default_preprocessor_cfg
    cfg = dict(default_preprocessor_cfg()['clip'], top_k=32)
    cfg['class_list'] = [f'c{i}' for i in range(40)]
    cfg['class_mapping'] = {c: 'Vehicle' for c in cfg['class_list']}
    assert no_tower(cfg, '/nonexistent', device='cpu').top_k == 32


@pytest.mark.parametrize('top_k', [0, -1, 33, True, False, 2.0, 1.5, '3', None, np.float32(2), np.bool_(True)])
def test_clipwrapper_refuses_top_k_outside_the_range(top_k):
    from vilgod_amd.clip_wrapper import ClipWrapper
    with pytest.raises(ValueError, match=r'clip\.top_k.*1 \.\. 32'):
        ClipWrapper(_clip_cfg(top_k), '/nonexistent', device='cpu')


def test_clipwrapper_refuses_more_top_k_than_classes():
    from vilgod_amd.clip_wrapper import ClipWrapper
    with pytest.raises(ValueError, match=r'clip\.top_k = 7 exceeds the 6 classes.*1 \.\. 6'):
        ClipWrapper(_clip_cfg(7), '/nonexistent', device='cpu')
