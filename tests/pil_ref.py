"""numpy restatement of PIL's 8-bit bicubic resample (Pillow src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc, then
ImagingResampleVertical_8bpc) with the tables of vilgod_amd/pil_resample.py, and of the float32 bilinear that precedes it in the
reference's chain (src/vilgod/zero_shot_detector.py:405-409).  tests/test_image_size_host.py pins both: the resample against PIL's
frozen hashes (and live PIL where it imports), the bilinear against torch's CPU `F.interpolate(..., align_corners=True)`.
"""
import hashlib

import numpy as np

from vilgod_amd import pil_resample as pr


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the seeded inputs of the resample tests (tests/golden/make_image_size.py freezes PIL's output for exactly these)
RESAMPLE_SIDES = [65, 223, 225, 256, 336, 447, 448]          # ksize 5 / 7 / 9, both sides of the filter-scale clamp at 224, odd and even
RESAMPLE_FAMILIES = ['uniform', 'sparse255', 'binary', 'constant', 'impulses']
CHAIN_SIZES = [65, 96, 223, 225, 336, 448]
CHAIN_SETTINGS = [(112, 8, 0.8, 0.2), (16, 8, 0.8, 0.2), (128, 8, 0.8, 0.2)]      # shipped, smallest and largest renderer resolution
CHAIN_CLUSTERS = [3, 4]                                       # originf32_k of render_params_golden.npz: 397 and 3011 points


def resample_inputs(side, family):
    """uint8 [3, side, side]: three different single-channel images of one family"""
    rng = np.random.default_rng(1000 * side + RESAMPLE_FAMILIES.index(family))
    shape = (3, side, side)
    if family == 'uniform':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if family == 'sparse255':                                 # negative lobes next to zeros: sums below 0, clamped
        return np.where(rng.random(shape) < 0.05, 255, 0).astype(np.uint8)
    if family == 'binary':                                    # overshoot next to 255: sums above 255, clamped
        return np.where(rng.random(shape) < 0.5, 255, 0).astype(np.uint8)
    if family == 'constant':                                  # the taps of every pixel sum to 2^22 within their rounding
        return np.stack([np.full((side, side), v, np.uint8) for v in (255, 1, 254)])
    a = np.zeros(shape, np.uint8)                             # impulses: the four corners, the centre, all five
    for y, x in ((0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1)):
        a[0, y, x] = a[2, y, x] = 255
    a[1, side // 2, side // 2] = a[2, side // 2, side // 2] = 255
    return a


def _pass(img, bounds, coef):
    """one pass along the LAST axis: uint8 [..., in] -> uint8 [..., out]; int64 sums (the int32 bound is a test of its own)"""
    out = np.empty(img.shape[:-1] + (len(bounds),), np.uint8)
    wide = img.astype(np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        ss = (wide[..., xmin:xmin + cnt] * coef[xx, :cnt].astype(np.int64)).sum(-1) + (1 << (pr.PRECISION_BITS - 1))
        out[..., xx] = np.clip(ss >> pr.PRECISION_BITS, 0, 255)            # clip8: arithmetic shift, then clamp
    return out


def resize_bicubic(u8, out_side=pr.OUT_SIDE):
    """uint8 [..., S, S] -> uint8 [..., out, out] = Image.resize((out, out), Image.BICUBIC) of every image: horizontal, then vertical"""
    u8 = np.asarray(u8, np.uint8)
    bounds, coef, _ = pr.bicubic_coeffs(u8.shape[-1], out_side)
    h = _pass(u8, bounds, coef)                                                # [..., S, out]
    if u8.shape[-2] != u8.shape[-1]:
        bounds, coef, _ = pr.bicubic_coeffs(u8.shape[-2], out_side)
    return np.swapaxes(_pass(np.swapaxes(h, -1, -2), bounds, coef), -1, -2)


def bilinear_tables(G, S):
    """source index and weights of F.interpolate(align_corners=True) from side G to side S as csrc/render.hip forms them in float32"""
    scale = np.float32(G - 1) / np.float32(S - 1)
    src = scale * np.arange(S, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int32), G - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    i1 = i0 + (i0 < G - 1)
    return i0, i1, l0.astype(np.float32), l1.astype(np.float32)


def _fma(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, rounded once.  The product is exact in float64 (two 24-bit factors); its sum with c can
    need more than 53 bits, so the float64 sum is turned into the round-to-odd one (TwoSum gives the exact error; an inexact sum with
    an even last bit moves one ulp towards the error) before it is rounded to float32: 53 >= 24 + 2 bits make that the single rounding."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64)
    toward = np.where((err > 0) == (s > 0), 1, -1)
    bits = np.where((err != 0) & ((bits & 1) == 0), bits + toward, bits)
    return bits.view(np.float64).astype(np.float32)


def bilinear(img, S):
    """float32 [n, G, G] (one channel of get_img) -> float32 [n, S, S] = F.interpolate(img, (S, S), 'bilinear', align_corners=True):
    fma(p00, lw0, p01 * lw1) along W, then fma(t0, lh0, t1 * lh1) along H, each product rounded on its own (csrc/render.hip)."""
    img = np.asarray(img, np.float32)
    G = img.shape[-1]
    i0, i1, l0, l1 = bilinear_tables(G, S)
    top, bot = img[:, i0], img[:, i1]                                          # [n, S(h), G]
    def row(r):
        return _fma(r[:, :, i0], l0[None, None, :], (r[:, :, i1] * l1[None, None, :]).astype(np.float32))
    t0, t1 = row(top), row(bot)
    return _fma(t0, l0[None, :, None], (t1 * l1[None, :, None]).astype(np.float32))


def chain(img, S):
    """one channel of get_img, float32 [n, G, G] -> the uint8 [n, 224, 224] CLIP's Resize sees first: bilinear to S, the H <-> W swap
    of permute(0, 3, 2, 1), np.uint8(x * 255), PIL's resample (zero_shot_detector.py:405-410, clip.py:79-86)"""
    big = np.swapaxes(bilinear(img, S), -1, -2)
    u8 = np.clip((big * np.float32(255.0)).astype(np.int32), 0, 255).astype(np.uint8)
    return resize_bicubic(u8)
