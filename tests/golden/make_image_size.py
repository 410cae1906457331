"""Generates tests/golden/image_size_golden.npz: what PIL and the REFERENCE's own chain produce for `classification.image_size` other
than 224.  Run only where Pillow and the reference checkout exist (stub-imported, see oracle/refstubs.py):

    python tests/golden/make_image_size.py

The fixture holds hashes, no images and no reference source:
  pil_hashes [side, family]            sha256 of Image.resize((224, 224), Image.BICUBIC) of the seeded uint8 images of
                                       tests/pil_ref.py::resample_inputs (three images per case, channel 0 of the RGB result)
  chain_hashes [setting, size, cluster] sha256 of the four crops of a cluster as CLIP's Resize leaves them: `mv_utils.RealisticProjection
                                       (cfg).get_img` on the frozen origin points of render_params_golden.npz (the four views as one
                                       batch), F.interpolate to image_size, permute, np.uint8(img * 255) (zero_shot_detector.py:405-409),
                                       Image.fromarray(...).resize((224, 224), Image.BICUBIC) (clip.py:79-86 Resize on a square image)
  and the lists that index them, plus Pillow's version.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image, __version__ as PIL_VERSION

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refstubs  # noqa: E402
import pil_ref  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def pil_resize(gray):
    """uint8 [S, S] -> uint8 [224, 224]: the grey image as the RGB array the reference hands to PIL; the channels come back equal"""
    rgb = np.repeat(gray[..., None], 3, axis=-1)
    out = np.asarray(Image.fromarray(rgb).resize((224, 224), Image.BICUBIC))
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    return out[..., 0]


def main():
    pil_hashes = []
    for side in pil_ref.RESAMPLE_SIDES:
        for family in pil_ref.RESAMPLE_FAMILIES:
            want = np.stack([pil_resize(x) for x in pil_ref.resample_inputs(side, family)])
            assert np.array_equal(pil_ref.resize_bicubic(pil_ref.resample_inputs(side, family)), want), (side, family)
            pil_hashes.append(pil_ref.sha(want))

    refstubs.install()
    from src.utils import mv_utils
    g = np.load(os.path.join(OUT, 'render_params_golden.npz'))
    chain_hashes, restated = [], 0
    for (R, D, ratio, bias) in pil_ref.CHAIN_SETTINGS:
        cfg = refstubs.projection_cfg()
        cfg.resolution, cfg.depth, cfg.obj_ratio, cfg.depth_bias = R, D, ratio, bias
        proj = mv_utils.RealisticProjection(cfg)
        imgs = {k: proj.get_img(torch.from_numpy(g[f'originf32_{k}']).unsqueeze(0)).detach() for k in pil_ref.CHAIN_CLUSTERS}
        for S in pil_ref.CHAIN_SIZES:
            for k in pil_ref.CHAIN_CLUSTERS:
                img = imgs[k]                                                       # [4, 3, R-2, R-2]: the four views as one batch
                big = torch.nn.functional.interpolate(img, size=(S, S), mode='bilinear', align_corners=True)
                big = big.permute(0, 3, 2, 1).detach().cpu().numpy()               # zero_shot_detector.py:405-408
                u8 = np.stack([np.uint8(b * 255) for b in big])                    # :409
                assert (u8[..., 0] == u8[..., 1]).all() and (u8[..., 0] == u8[..., 2]).all()
                out = np.stack([np.asarray(Image.fromarray(x).resize((224, 224), Image.BICUBIC)) for x in u8])
                assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
                restated += int(np.array_equal(pil_ref.chain(img[:, 0].numpy(), S), out[..., 0]))
                chain_hashes.append(pil_ref.sha(out[..., 0]))
    n_s, n_z, n_k = len(pil_ref.CHAIN_SETTINGS), len(pil_ref.CHAIN_SIZES), len(pil_ref.CHAIN_CLUSTERS)
    path = os.path.join(OUT, 'image_size_golden.npz')
    np.savez_compressed(
        path, pillow=np.array(PIL_VERSION), sides=np.array(pil_ref.RESAMPLE_SIDES), families=np.array(pil_ref.RESAMPLE_FAMILIES),
        pil_hashes=np.array(pil_hashes).reshape(len(pil_ref.RESAMPLE_SIDES), len(pil_ref.RESAMPLE_FAMILIES)),
        settings=np.array(pil_ref.CHAIN_SETTINGS, dtype=np.float64), sizes=np.array(pil_ref.CHAIN_SIZES),
        clusters=np.array(pil_ref.CHAIN_CLUSTERS), chain_hashes=np.array(chain_hashes).reshape(n_s, n_z, n_k))
    print('image_size_golden.npz', len(pil_hashes), 'resample cases,', len(chain_hashes), 'chain cases (the restatement equals',
          restated, 'of them),', os.path.getsize(path), 'bytes, Pillow', PIL_VERSION)


if __name__ == '__main__':
    main()
