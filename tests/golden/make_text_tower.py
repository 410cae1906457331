"""Generates tests/golden/text_tower_golden.npz: the REFERENCE's CLIP.encode_text (third_party/CLIP/clip/model.py:343-356, imported
through oracle/refstubs.py as the text section of make_golden.py does) in fp32 on the CPU, on a seeded TWO-head text tower
(clip_weights.synthetic_text_weights: width 128, 2 layers, embed 64) and hand-made token rows -- no BPE file involved:

  sot, random ids below 49406, eot at positions 1, 2, 31, 32, 33, 63, 64, 65, 76, 7, 8, 17, zero padding   (12 rows)
  one row (eot at 20) whose padding after eot holds random ids below 49406                                (1 row)

Only data is stored: tokens, features, the sizes and the seed.

    python tests/golden/make_text_tower.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refstubs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SOT, EOT, CTX = 49406, 49407, 77
EOT_POSITIONS = (1, 2, 31, 32, 33, 63, 64, 65, 76, 7, 8, 17)


def main():
    from vilgod_amd import clip_weights as cw
    from text_tower_ref import make_tokens
    width, layers, heads, embed, seed = 128, 2, 2, 64, 0
    tokens = make_tokens(EOT_POSITIONS, seed=20, dirty_rows=(20,))
    m = refstubs.load_clip_model_py()
    model = m.CLIP(embed_dim=embed, image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=16, context_length=CTX,
                   vocab_size=49408, transformer_width=width, transformer_heads=heads, transformer_layers=layers)
    sd = cw.synthetic_text_weights(seed, width=width, layers=layers, embed=embed)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('visual.') or k == 'logit_scale' for k in missing), (missing, unexpected)
    model = model.float().eval()
    with torch.no_grad():
        feat = model.encode_text(torch.from_numpy(tokens)).numpy()
    np.savez_compressed(os.path.join(OUT, 'text_tower_golden.npz'), tokens=tokens, features=feat, width=width, layers=layers,
                        heads=heads, embed=embed, seed=seed)
    print('text_tower_golden.npz', tokens.shape, feat.shape, 'max |feature|', float(np.abs(feat).max()))


if __name__ == '__main__':
    main()
