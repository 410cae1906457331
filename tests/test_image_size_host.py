"""`classification.image_size` other than 224, host side (no GPU):
  * tests/pil_ref.py (the numpy restatement the GPU tests compare against) reproduces PIL's frozen hashes, and live PIL where it imports;
  * the int32 tables of vilgod_amd/pil_resample.py: rows sum to 2^22 within their rounding, 224 -> 224 is the identity, and
    sum |k| * 255 + 2^21 stays below 2^31 for every supported size (csrc/preprocess.hip accumulates in int32);
  * the restated bilinear equals torch's CPU F.interpolate(align_corners=True) from 65 upwards and differs at 64 -- why the range starts at 65;
  * the stage accepts 65 .. 448 and refuses the rest by name; the CLI override reaches it.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pil_ref
from conftest import ROOT
from vilgod_amd import config as vconfig
from vilgod_amd import pil_resample as pr


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(f'{golden_dir}/image_size_golden.npz')


def test_fixture_indexes_the_cases_of_pil_ref(golden):
    g = golden
    assert list(g['sides']) == pil_ref.RESAMPLE_SIDES and list(g['families']) == pil_ref.RESAMPLE_FAMILIES
    assert list(g['sizes']) == pil_ref.CHAIN_SIZES and list(g['clusters']) == pil_ref.CHAIN_CLUSTERS
    assert [tuple(s) for s in g['settings']] == pil_ref.CHAIN_SETTINGS
    assert g['pil_hashes'].shape == (7, 5) and g['chain_hashes'].shape == (3, 6, 2)
    assert len(set(g['pil_hashes'][:, :3].ravel())) == 21 and len(set(g['chain_hashes'].ravel())) == 36     # (a constant image resizes to itself)


@pytest.mark.parametrize('side', pil_ref.RESAMPLE_SIDES)
def test_restatement_reproduces_pils_frozen_hashes(golden, side):
    i = pil_ref.RESAMPLE_SIDES.index(side)
    for f, family in enumerate(pil_ref.RESAMPLE_FAMILIES):
        got = pil_ref.resize_bicubic(pil_ref.resample_inputs(side, family))
        assert got.shape == (3, 224, 224) and got.dtype == np.uint8
        assert pil_ref.sha(got) == golden['pil_hashes'][i, f], (side, family)


def test_restatement_equals_live_pil():
    try:
        from PIL import Image
    except ImportError:                   # Pillow is no dependency of the package: without it the frozen hashes above are the check
        return
    rng = np.random.default_rng(7)
    for side in (65, 150, 224, 299, 448):
        a = rng.integers(0, 256, (side, side), dtype=np.uint8)
        want = np.asarray(Image.fromarray(np.repeat(a[..., None], 3, -1)).resize((224, 224), Image.BICUBIC))
        assert (want[..., 0] == want[..., 1]).all() and (want[..., 0] == want[..., 2]).all()
        assert np.array_equal(pil_ref.resize_bicubic(a), want[..., 0]), side


def test_tables_rows_sum_to_one_within_their_rounding():
    for side in (65, 66, 223, 224, 225, 300, 336, 447, 448):
        bounds, coef, ksize = pr.bicubic_coeffs(side)
        assert bounds.shape == (224, 2) and coef.shape == (224, ksize) and bounds.dtype == coef.dtype == np.int32
        assert ksize == pr.ksize_for(side) and ksize <= 9
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= side).all() and (bounds[:, 1] <= ksize).all()
        for xx in range(224):
            assert not coef[xx, bounds[xx, 1]:].any()
        # each tap is rounded to the nearest integer on its own: the row misses 2^22 by at most half a unit per tap
        assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= bounds[:, 1] / 2.0).all(), side
    assert (pr.ksize_for(65), pr.ksize_for(224), pr.ksize_for(225), pr.ksize_for(336), pr.ksize_for(448)) == (5, 5, 7, 7, 9)


def test_side_224_is_the_identity():
    bounds, coef, _ = pr.bicubic_coeffs(224)
    for xx in range(224):
        row = np.zeros(224, np.int64)
        row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = coef[xx, :bounds[xx, 1]]
        assert row[xx] == 1 << 22 and np.count_nonzero(row) == 1
    a = np.random.default_rng(1).integers(0, 256, (2, 224, 224), dtype=np.uint8)
    assert np.array_equal(pil_ref.resize_bicubic(a), a)


def test_int32_accumulator_suffices_for_every_supported_size():
    worst = 0
    for side in range(pr.MIN_IMAGE_SIZE, pr.MAX_IMAGE_SIZE + 1):
        _, coef, _ = pr.bicubic_coeffs(side)
        worst = max(worst, int(np.abs(coef.astype(np.int64)).sum(1).max()) * 255 + (1 << 21))
    print(f'largest |sum| of a pass over 65 .. 448: {worst} = {worst / 2 ** 31:.3f} * 2^31')
    assert worst < 2 ** 31


def test_supported_range_is_the_headers():
    from vilgod_amd import _lib
    assert _lib.PREPROCESS_IMAGE_SIZE == (pr.MIN_IMAGE_SIZE, pr.MAX_IMAGE_SIZE) == (65, 448)


def _torch_interpolate(img, S):
    t = torch.from_numpy(img)[:, None].repeat(1, 3, 1, 1)                      # three equal channels, as get_img returns them
    return torch.nn.functional.interpolate(t, size=(S, S), mode='bilinear', align_corners=True)[:, 0].numpy()


def test_restated_bilinear_equals_torch_cpu_from_65_upwards_and_not_at_64():
    rng = np.random.default_rng(11)
    for G in (14, 110, 126):                                                    # renderer resolutions 16, 112, 128
        img = rng.random((4, G, G), dtype=np.float32)
        for S in pil_ref.CHAIN_SIZES + [224]:
            assert np.array_equal(pil_ref.bilinear(img, S), _torch_interpolate(img, S)), (G, S)
    # below 65 torch's CPU kernel sums in another order: the last bit differs in a good part of the values.  This difference is the
    # reason for the lower bound of the range; it is pinned so that a torch whose kernel changes shows up here.
    img = rng.random((4, 110, 110), dtype=np.float32)
    got, want = pil_ref.bilinear(img, 64), _torch_interpolate(img, 64)
    assert (got != want).mean() > 0.05 and np.abs(got - want).max() < 1e-6


def _stage_self(overrides=()):
    cfg = vconfig.load(os.path.join(ROOT, 'tools', 'configs'), 'preprocessing', ['preprocessor=waymo'] + list(overrides))
    return SimpleNamespace(cfg=cfg, pipe=SimpleNamespace(box_mode='fast'))


def test_stage_accepts_the_range_and_refuses_the_rest_by_name():
    from vilgod_amd.zero_shot_detector import ZeroShotDetector
    me = _stage_self()
    for size in (65, 224, 336, 448):
        assert ZeroShotDetector._classification_context(me, image_size=size)['image_size'] == size
    for size in (64, 449, 0, -224, 224.0, None, True):
        with pytest.raises(NotImplementedError, match=r'image_size.*65 \.\. 448'):
            ZeroShotDetector._classification_context(me, image_size=size)
    with pytest.raises(NotImplementedError, match='image_size.*voting'):
        ZeroShotDetector._classification_context(me, image_size=336, aggregation='mean')
    with pytest.raises(NotImplementedError, match='voting'):
        ZeroShotDetector._classification_context(me, aggregation='mean')


def test_cli_override_reaches_the_stage():
    from vilgod_amd.zero_shot_detector import ZeroShotDetector
    me = _stage_self(['pipeline.5.args.image_size=336'])
    task = me.cfg.pipeline[5]
    assert task['name'] == 'classification' and task['args']['image_size'] == 336
    assert ZeroShotDetector._classification_context(me, **task['args'])['image_size'] == 336
    assert ZeroShotDetector._classification_context(_stage_self(), **_stage_self().cfg.pipeline[5]['args'])['image_size'] == 224
    with pytest.raises(NotImplementedError, match='image_size'):
        bad = _stage_self(['pipeline.5.args.image_size=64'])
        ZeroShotDetector._classification_context(bad, **bad.cfg.pipeline[5]['args'])


def test_pipeline_and_projection_refuse_sizes_outside_the_range():
    from vilgod_amd.projection import check_image_size
    assert [check_image_size(s) for s in (65, 224, np.int64(448))] == [65, 224, 448]
    for size in (64, 449, 0, 336.0):
        with pytest.raises(NotImplementedError, match='image_size'):
            check_image_size(size)


def test_new_kernel_uses_no_scratch():
    from vilgod_amd import build
    assert build.check_scratch('preprocess.hip', '') == []
    assert build.check_isa(sources=['preprocess.hip']) == []
