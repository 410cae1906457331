"""References of the device text tower's tests (tests/test_text_tower.py) and of the fixture generator tests/golden/make_text_tower.py:
hand-made token rows, CLIP.encode_text restated in float64 (third_party/CLIP/clip/model.py:343-356 as vilgod_amd/clip_text.encode_text
reads it), and the float64 masked softmax(q k^T / 8) v of the causal attention kernels in the layout of tests/attention_ref.py."""
import numpy as np
import torch

SOT, EOT, CTX = 49406, 49407, 77
EOT_POSITIONS = (1, 2, 31, 32, 33, 63, 64, 65, 76, 7, 8, 17)


def make_tokens(eot_positions=EOT_POSITIONS, seed=20, dirty_rows=(), ctx=CTX):
    """int64 [len(eot_positions) + len(dirty_rows), ctx]: sot, random ids below 49406, eot at the given position, zero padding; the
    rows of `dirty_rows` (their eot positions) carry random ids below 49406 behind eot instead of zeros.  No tokenizer involved."""
    g = np.random.default_rng(seed)
    rows = [(e, False) for e in eot_positions] + [(e, True) for e in dirty_rows]
    tok = np.zeros((len(rows), ctx), np.int64)
    for r, (e, dirty) in enumerate(rows):
        assert 1 <= e < ctx
        tok[r, 0] = SOT
        tok[r, 1:e] = g.integers(1, SOT, e - 1)
        tok[r, e] = EOT
        if dirty:
            tok[r, e + 1:] = g.integers(1, SOT, ctx - e - 1)
    return tok


def eot_of(tokens):
    """the first maximum of every row: torch's argmax, as model.py:354"""
    return torch.as_tensor(np.asarray(tokens)).long().argmax(dim=-1)


@torch.no_grad()
def encode_text_f64(sd, tokens):
    """CLIP.encode_text in float64 throughout -> float64 [n, embed] (not normalised)."""
    sd = {k: v.double() for k, v in sd.items()}
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long)
    x = sd['token_embedding.weight'][tok] + sd['positional_embedding'][:tok.shape[1]]
    n, L, W = x.shape
    H = max(W // 64, 1)
    dh = W // H
    mask = torch.full((L, L), float('-inf'), dtype=torch.float64).triu_(1)
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (W,), sd[p + '.weight'], sd[p + '.bias'], 1e-5)
    layers = len([k for k in sd if k.endswith('attn.in_proj_weight')])
    for i in range(layers):
        p = f'transformer.resblocks.{i}.'
        qkv = ln(x, p + 'ln_1') @ sd[p + 'attn.in_proj_weight'].t() + sd[p + 'attn.in_proj_bias']
        q, k, v = (t.reshape(n, L, H, dh).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
        a = torch.softmax((q * dh ** -0.5) @ k.transpose(-1, -2) + mask, dim=-1) @ v
        x = x + a.transpose(1, 2).reshape(n, L, W) @ sd[p + 'attn.out_proj.weight'].t() + sd[p + 'attn.out_proj.bias']
        h = ln(x, p + 'ln_2') @ sd[p + 'mlp.c_fc.weight'].t() + sd[p + 'mlp.c_fc.bias']
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ sd[p + 'mlp.c_proj.weight'].t() + sd[p + 'mlp.c_proj.bias']
    x = ln(x, 'ln_final')
    return x[torch.arange(n), tok.argmax(dim=-1)] @ sd['text_projection']


def causal_reference(qkv, n_items, T, W, H):
    """float64 masked softmax(q k^T / 8) v (row q sees keys 0 .. q) of the given fp16 / fp32 input bits, in attention_ref's layouts.
    -> (want, A) [n_items * T, W] float64, A = softmax(...) |v| as attention_ref.reference returns it."""
    import attention_ref as R
    q, k, v = R._heads(qkv, n_items, T, W, H)
    mask = torch.full((T, T), float('-inf'), dtype=torch.float64).triu_(1)
    want, A = torch.empty_like(q), torch.empty_like(q)
    for c in range(n_items):
        p = torch.softmax(q[c] @ k[c].transpose(-1, -2) * 0.125 + mask, dim=-1)
        want[c] = p @ v[c]
        A[c] = p @ v[c].abs()
    return R._rows(want), R._rows(A)
