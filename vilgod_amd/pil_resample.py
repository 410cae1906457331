"""Coefficient tables of PIL's antialiased bicubic resample of 8-bit images (Pillow src/libImaging/Resample.c), computed on the host.

CLIP's `preprocess` (third_party/CLIP/clip/clip.py:79-86) opens with `Resize(224, BICUBIC)` on the PIL image the reference builds at
src/vilgod/zero_shot_detector.py:405-410.  For a square `image_size` image that is `Image.resize((224, 224), Image.BICUBIC)`: one
horizontal and one vertical pass with the same table, each `clip8((2^21 + sum pixel * k) >> 22)` on int32 coefficients.  The table is
`precompute_coeffs` followed by `normalize_coeffs_8bpc`, restated here in Python floats (C doubles): the same operations in the same
order, so the integers are PIL's.  csrc/preprocess.hip (vg_clip_preprocess) and tests/pil_ref.py consume it.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2          # Resample.c: 8 bits of pixel, 2 bits of head room for the negative lobes
SUPPORT = 2.0                        # bicubic filter support
OUT_SIDE = 224                       # CLIP input side
MIN_IMAGE_SIZE, MAX_IMAGE_SIZE = 65, 448


def bicubic_filter(x):
    """Resample.c bicubic_filter, a = -0.5 (Keys)"""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_for(in_size, out_size=OUT_SIDE):
    """taps per output pixel that precompute_coeffs reserves: ceil(support * max(scale, 1)) * 2 + 1"""
    filterscale = max(float(in_size) / out_size, 1.0)
    return int(math.ceil(SUPPORT * filterscale)) * 2 + 1


def bicubic_coeffs(in_size, out_size=OUT_SIDE):
    """-> (bounds int32 [out,2] = (first input pixel, tap count), coef int32 [out,ksize], ksize) of one pass from in_size to out_size."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError('sizes must be positive')
    filterscale = scale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        ww = 0.0
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)               # (int) truncates towards zero, like C
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        for x in range(xmax):
            w = bicubic_filter((x + xmin - center + 0.5) * ss)
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        for x in range(ksize):                            # normalize_coeffs_8bpc
            coef[xx, x] = int(-0.5 + k[x] * one) if k[x] < 0 else int(0.5 + k[x] * one)
        bounds[xx] = (xmin, xmax)
    return bounds, coef, ksize
