"""Text side of `ClipWrapper.__init__`: the 24 prompts -> L2-normalised text features, computed ONCE at
start-up with plain torch (not a kernel, not on the hot path) and cached next to the checkpoint -- or, with tower='device' /
`TextTower`, by the text tower of the C ABI on the GPU (vg_text_*, csrc/vit_text.inc), which long class lists want.

Mirrors
  clip.tokenize                     third_party/CLIP/clip/clip.py:197-237        (sot + BPE + eot, zero padded to 77)
  SimpleTokenizer                   third_party/CLIP/clip/simple_tokenizer.py:62-132 (byte-level BPE over the shipped merges file)
  CLIP.encode_text                  third_party/CLIP/clip/model.py:343-356       (token + positional embedding, causal
                                    transformer of ResidualAttentionBlocks :171-192, ln_final, row of the eot token @ text_projection)
  ClipWrapper.__init__ text side    src/utils/clip_utils.py:22-26                (prompt_template.format(cls), normalise)

The merges file `bpe_simple_vocab_16e6.txt.gz` is data of the CLIP package the reference vendors; it is looked up next to an
installed `clip` package (the reference's PYTHONPATH contract, README.md:130-133) or taken from `bpe_path`.
"""
import gzip
import html
import importlib.util
import os

import numpy as np
import torch


def find_bpe_vocab(bpe_path=None):
    if bpe_path and os.path.exists(bpe_path):
        return bpe_path
    spec = importlib.util.find_spec('clip')                     # locates the package without importing it
    if spec is not None and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], 'bpe_simple_vocab_16e6.txt.gz')
        if os.path.exists(p):
            return p
    return None


def _byte_alphabet():
    """The reversible byte <-> printable-unicode table of the GPT-2 / CLIP BPE."""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(ord('¡'), ord('¬') + 1)) + list(range(ord('®'), ord('ÿ') + 1))
    table, extra = {}, 0
    for b in keep:
        table[b] = chr(b)
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + extra)
            extra += 1
    order = keep + [b for b in range(256) if b not in keep]
    return table, [table[b] for b in order]


class BpeTokenizer:
    def __init__(self, bpe_path):
        import regex
        self.byte_to_char, alphabet = _byte_alphabet()
        with gzip.open(bpe_path) as f:
            lines = f.read().decode('utf-8').split('\n')
        merges = [tuple(l.split()) for l in lines[1:49152 - 256 - 2 + 1]]
        vocab = alphabet + [c + '</w>' for c in alphabet] + [''.join(m) for m in merges] + ['<|startoftext|>', '<|endoftext|>']
        self.token_id = {t: i for i, t in enumerate(vocab)}
        self.rank = {m: i for i, m in enumerate(merges)}
        self.sot, self.eot = self.token_id['<|startoftext|>'], self.token_id['<|endoftext|>']
        self.word_re = regex.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
                                     regex.IGNORECASE)
        self._ws_re = regex.compile(r'\s+')
        self._cache = {}

    def _merge(self, word):
        """Greedy BPE: repeatedly join the adjacent pair with the lowest merge rank."""
        if word in self._cache:
            return self._cache[word]
        parts = list(word[:-1]) + [word[-1] + '</w>']
        while len(parts) > 1:
            ranked = [(self.rank.get((a, b), None), i) for i, (a, b) in enumerate(zip(parts[:-1], parts[1:]))]
            ranked = [(r, i) for r, i in ranked if r is not None]
            if not ranked:
                break
            best = min(ranked)[0]
            first, second = next((a, b) for a, b in zip(parts[:-1], parts[1:]) if self.rank.get((a, b)) == best)
            out, i = [], 0
            while i < len(parts):
                if i < len(parts) - 1 and parts[i] == first and parts[i + 1] == second:
                    out.append(first + second)
                    i += 2
                else:
                    out.append(parts[i])
                    i += 1
            parts = out
        self._cache[word] = parts
        return parts

    def encode(self, text):
        if not text.isascii():
            try:
                import ftfy
                text = ftfy.fix_text(text)
            except ImportError as e:
                raise RuntimeError('non-ASCII prompt: the reference cleans it with ftfy, which is not installed') from e
        text = html.unescape(html.unescape(text)).strip()
        text = self._ws_re.sub(' ', text).strip().lower()
        ids = []
        for w in self.word_re.findall(text):
            chars = ''.join(self.byte_to_char[b] for b in w.encode('utf-8'))
            ids.extend(self.token_id[p] for p in self._merge(chars))
        return ids


def tokenize(tokenizer, texts, context_length=77):
    """-> int64 [n, context_length]: sot, BPE ids, eot, zero padding (clip.py:197-237, truncate=False)."""
    out = np.zeros((len(texts), context_length), np.int64)
    for i, t in enumerate(texts):
        ids = [tokenizer.sot] + tokenizer.encode(t) + [tokenizer.eot]
        if len(ids) > context_length:
            raise RuntimeError(f'Input {t} is too long for context length {context_length}')
        out[i, :len(ids)] = ids
    return out


def load_text_state_dict(path):
    """The text-tower tensors of a CLIP checkpoint (TorchScript archive or plain state dict), float32."""
    try:
        sd = torch.jit.load(path, map_location='cpu').state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location='cpu')
    keep = ('token_embedding.', 'positional_embedding', 'transformer.', 'ln_final.', 'text_projection')
    return {k: v.float() for k, v in sd.items() if k.startswith(keep)}


@torch.no_grad()
def encode_text(sd, tokens, device='cpu'):
    """model.py:343-356 on a state dict.  tokens int64 [n, ctx] -> float32 [n, embed] (NOT normalised)."""
    sd = {k: v.to(device=device, dtype=torch.float32) for k, v in sd.items()}
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long, device=device)
    x = sd['token_embedding.weight'][tok] + sd['positional_embedding'][:tok.shape[1]]
    n, L, W = x.shape
    heads = max(W // 64, 1)
    dh = W // heads
    mask = torch.full((L, L), float('-inf'), device=device).triu_(1)                # model.py:320-326 build_attention_mask
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (W,), sd[p + '.weight'], sd[p + '.bias'], 1e-5)
    layers = len([k for k in sd if k.endswith('attn.in_proj_weight')])
    for i in range(layers):
        p = f'transformer.resblocks.{i}.'
        h = ln(x, p + 'ln_1')
        qkv = h @ sd[p + 'attn.in_proj_weight'].t() + sd[p + 'attn.in_proj_bias']
        q, k, v = (t.reshape(n, L, heads, dh).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
        a = torch.softmax((q * dh ** -0.5) @ k.transpose(-1, -2) + mask, dim=-1) @ v
        a = a.transpose(1, 2).reshape(n, L, W)
        x = x + a @ sd[p + 'attn.out_proj.weight'].t() + sd[p + 'attn.out_proj.bias']
        h = ln(x, p + 'ln_2')
        h = h @ sd[p + 'mlp.c_fc.weight'].t() + sd[p + 'mlp.c_fc.bias']
        h = h * torch.sigmoid(1.702 * h)                                              # QuickGELU, model.py:166-168
        x = x + h @ sd[p + 'mlp.c_proj.weight'].t() + sd[p + 'mlp.c_proj.bias']
    x = ln(x, 'ln_final')
    eot = tok.argmax(dim=-1)                                                          # the eot token has the highest id
    return (x[torch.arange(n, device=device), eot] @ sd['text_projection']).float().cpu()


def text_config(sd):
    """The text tower's sizes, read from its tensors (model.py:288-300)."""
    vocab, width = sd['token_embedding.weight'].shape
    layers = len([k for k in sd if k.startswith('transformer.resblocks.') and k.endswith('attn.in_proj_weight')])
    return {'width': int(width), 'layers': layers, 'heads': max(int(width) // 64, 1), 'ctx': int(sd['positional_embedding'].shape[0]),
            'vocab': int(vocab), 'output_dim': int(sd['text_projection'].shape[1])}


class TextTower:
    """CLIP.encode_text (model.py:343-356) on the device: owns a vg_text handle (include/vilgod_hip.h) and one workspace sized for a
    chunk of prompts.  dtype 'f32' is the parity mode, 'f16' the fp16 tower on the fp32 stream."""

    CHUNK = 256          # prompts per vg_text_encode: 256 x 77 rows are exactly 77 row tiles of the projection GEMMs

    def __init__(self, state_dict, dtype='f32', device='cuda'):
        import ctypes
        from ._lib import lib, check
        keep = ('token_embedding.', 'positional_embedding', 'transformer.', 'ln_final.', 'text_projection')
        sd = {k: v for k, v in state_dict.items() if k.startswith(keep)}
        self.cfg = text_config(sd)
        self.dtype = dtype
        self.device = torch.device(device)
        self._h = None
        h = ctypes.c_void_p()
        c = self.cfg
        check(lib.vg_text_create(ctypes.byref(h), c['width'], c['layers'], c['heads'], c['ctx'], c['vocab'], c['output_dim'],
                                 {'f32': 0, 'f16': 1}[dtype]), 'vg_text_create')
        self._h = h
        with torch.cuda.device(self.device):
            for name, t in sd.items():
                t = t.detach().to(torch.float32).contiguous().cpu()
                check(lib.vg_text_set_weight(self._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), f'vg_text_set_weight({name})')
        self._ws = None
        self._ws_prompts = 0

    def close(self):
        """Destroys the handle (the token table alone is 100 to 150 MB) and drops the workspace."""
        from ._lib import lib
        h, self._h = getattr(self, '_h', None), None
        if h is not None and lib is not None:
            lib.vg_text_destroy(h)
        self._ws = None

    __del__ = close

    def _workspace(self, n):
        from ._lib import lib
        if self._ws is None or n > self._ws_prompts:
            self._ws = None
            self._ws = torch.zeros(int(lib.vg_text_workspace_bytes(self._h, n)), dtype=torch.uint8, device=self.device)
            self._ws_prompts = n
        return self._ws

    def encode_chunk(self, tokens, eot, stream=None):
        """One vg_text_encode: tokens int32 [n, ctx] and eot int32 [n] on the device -> float32 [n, embed]."""
        from ._lib import lib, ptr, stream_ptr, check
        n = tokens.shape[0]
        feat = torch.empty((n, self.cfg['output_dim']), dtype=torch.float32, device=self.device)
        if n:
            with torch.cuda.device(self.device):
                check(lib.vg_text_encode(self._h, ptr(tokens), ptr(eot), n, ptr(self._workspace(n)), ptr(feat), stream_ptr(stream)), 'vg_text_encode')
        return feat

    def encode(self, tokens, stream=None):
        """tokens: integer [n, ctx] (numpy or torch) -> float32 [n, embed] on the device, NOT normalised, in chunks of CHUNK prompts."""
        tok = torch.as_tensor(np.asarray(tokens.cpu() if torch.is_tensor(tokens) else tokens)).long()
        assert tok.ndim == 2 and tok.shape[1] == self.cfg['ctx'], (tuple(tok.shape), self.cfg['ctx'])
        eot = tok.argmax(dim=-1).to(torch.int32).to(self.device)           # the first maximum: torch's argmax, as model.py:354
        tok = tok.to(torch.int32).to(self.device).contiguous()
        if tok.shape[0] > self.CHUNK:
            self._workspace(self.CHUNK)
        out = [self.encode_chunk(tok[i:i + self.CHUNK], eot[i:i + self.CHUNK], stream) for i in range(0, tok.shape[0], self.CHUNK)]
        return torch.cat(out) if out else torch.empty((0, self.cfg['output_dim']), dtype=torch.float32, device=self.device)


def tokenize_prompts(prompts, bpe_path=None):
    vocab = find_bpe_vocab(bpe_path)
    if vocab is None:
        raise FileNotFoundError('bpe_simple_vocab_16e6.txt.gz not found: put third_party/CLIP on PYTHONPATH (README.md:130-133 '
                                'of the reference) or pass its path (paths.clip_bpe)')
    return tokenize(BpeTokenizer(vocab), list(prompts))


def text_features(ckpt_path, prompts, bpe_path=None, device='cpu', tower='host'):
    """clip_utils.py:22-26: normalised features of the prompts (float32 [n, embed]; the reference computes them in the
    model's dtype -- fp16 on a GPU -- so its values differ from these in the 3rd-4th digit).  tower='device': the same tokens through
    fp32 TextTower on `device` (a CUDA device; 'cpu' means the current one) instead of the host's torch."""
    if tower not in ('host', 'device'):
        raise ValueError(f"tower must be 'host' or 'device', not {tower!r}")
    tok = tokenize_prompts(prompts, bpe_path)
    if tower == 'device':
        t = TextTower(load_text_state_dict(ckpt_path), dtype='f32', device='cuda' if str(device) == 'cpu' else device)
        try:
            f = t.encode(tok).cpu()
        finally:
            t.close()
    else:
        f = encode_text(load_text_state_dict(ckpt_path), tok, device=device)
    return (f / f.norm(dim=-1, keepdim=True)).numpy()
