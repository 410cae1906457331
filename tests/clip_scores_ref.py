"""float64 reference and seeded inputs for the scores head (vg_clip_scores / vg_clip_scores_wide, clip_utils.py:42-61), shared by the
tests of tests/test_class_list.py.  The inputs are those of tests/test_attention.py::test_clip_scores_shapes: the same seed rule, the
same draws in the same order."""
import functools
import zlib

import torch

N_CROPS = 37
SCALES = (1.0, 1e-4, 1e4)


def seed(*key):
    return zlib.crc32(repr(key).encode())


def unit_rows(n, dim, g):
    t = torch.randn(n, dim, generator=g)
    return t / t.norm(dim=-1, keepdim=True)


def reference(feat, text):
    """softmax(100 normalise(feat) text^T) in float64."""
    f = feat.double()
    return torch.softmax(100.0 * (f / f.norm(dim=-1, keepdim=True)) @ text.double().t(), dim=-1)


def inputs(dim, n_classes, scale):
    """-> (feat [37, dim], text [n_classes, dim]) float32 on the host."""
    g = torch.Generator().manual_seed(seed(dim, n_classes))
    feat = torch.randn(N_CROPS, dim, generator=g) * scale
    return feat, unit_rows(n_classes, dim, g)


@functools.lru_cache(maxsize=None)
def case(dim, n_classes, scale):
    """-> (feat, text, float64 probabilities), computed once per case and left unchanged by the tests that share it."""
    feat, text = inputs(dim, n_classes, scale)
    return feat, text, reference(feat, text)


def check_top1(probs, top1, score, want, margin=2e-5):
    """score is probs[top1] bit for bit, nothing exceeds it, and top1 is the reference's winner wherever that one leads by `margin`."""
    assert torch.equal(score, probs.gather(1, top1.long()[:, None])[:, 0])
    assert bool((probs <= score[:, None]).all())
    best2 = want.topk(2, dim=-1).values
    sure = best2[:, 0] - best2[:, 1] > margin
    assert torch.equal(top1.long()[sure], want.argmax(-1)[sure])
