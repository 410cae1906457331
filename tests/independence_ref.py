"""Shared pieces of tests/test_crop_independence.py and tests/test_graph_cache.py: the poison patterns, the clean / poison masks and
the check that a mask leaves no unit without poisoned neighbours, the one comparison every independence test goes through, a
restatement of the encode plan's choice of stream form (csrc/vit.hip vit_plan), and a model of the graph cache's counters
(csrc/vit_graph.inc).

The claim under test: a unit's numbers (a GEMM row, an attention item, a crop, a feature row) do not depend on which units share its
launch.  Every test runs one launch shape twice -- all units clean, and every other unit replaced by poison -- and compares the clean
units bit for bit.  Poison makes a leak categorical: NaN and Inf survive every sum, maximum and product they enter, the largest finite
value overflows the first sum it enters.  Nothing here has a tolerance."""
import torch

import vit_stages_ref as VS

POISONS = ('nan', 'inf', 'max')              # quiet NaN; +Inf / -Inf alternating by column; the largest finite value of the type
SCORE_POISONS = ('nan', 'inf', 'zero')       # feature rows of the scores kernels: a zero row has norm 0
TILE = 256                                   # rows per tile of the projection GEMMs


def bits(t):
    """The tensor's bit patterns as integers (NaN == NaN, -0 != +0)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def poison_row(ncols, dtype, kind, device='cpu'):
    """One row of poison [ncols]."""
    if kind == 'nan':
        return torch.full((ncols,), float('nan'), dtype=dtype, device=device)
    if kind == 'inf':
        sign = torch.where(torch.arange(ncols, device=device) % 2 == 0, 1.0, -1.0)
        return (sign * float('inf')).to(dtype)
    if kind == 'max':
        return torch.full((ncols,), torch.finfo(dtype).max, dtype=dtype, device=device)
    assert kind == 'zero', kind
    return torch.zeros((ncols,), dtype=dtype, device=device)


def with_poison(t, clean, kind):
    """A copy of t [rows, ...] whose rows with clean == False hold poison (clean: bool [rows], or a bool tensor that broadcasts against
    t.reshape(rows, -1))."""
    flat = t.reshape(t.shape[0], -1)
    clean = clean.to(t.device)
    if clean.dim() == 1:
        clean = clean[:, None]
    return torch.where(clean, flat, poison_row(flat.shape[1], t.dtype, kind, t.device)[None, :]).reshape(t.shape)


# ---------------------------------------------------------------------------------------------------------------------- masks
def unit_mask(n_units, phase):
    """bool [n_units], True = clean: units of parity `phase` are clean, the others poisoned.  The two phases are complementary."""
    return (torch.arange(n_units) % 2) == phase


def row_mask(M, gran, phase):
    """Clean rows of a launch of M rows whose units are runs of `gran` rows."""
    return unit_mask((M + gran - 1) // gran, phase).repeat_interleave(gran)[:M]


def crop_rows(n, rows_per_crop, phase, total=None):
    """Clean rows of n crops of rows_per_crop rows each; rows behind the last crop up to `total` (a buffer's padding rows) are poisoned."""
    m = unit_mask(n, phase).repeat_interleave(rows_per_crop)
    if total is not None:
        m = torch.cat([m, torch.zeros(total - m.numel(), dtype=torch.bool)])
    return m


def mask_gaps(clean_rows, gran):
    """What a mask leaves uncovered, as a list of strings (empty = nothing): a clean unit with a clean neighbour, and a 256-row tile that
    holds rows of more than one unit, a clean one among them, but no poisoned row.  (A tile that lies inside ONE unit -- T = 257: rows 0 .. 255
    are crop 0's -- holds whatever that unit holds; it is poisoned under the other phase.)"""
    M = clean_rows.numel()
    unit = torch.arange(M) // gran
    state = clean_rows[::gran]                              # one entry per unit
    gaps = [f'unit {int(u)} is partly poisoned' for u in unit[clean_rows != state[unit]].unique()]
    gaps += [f'clean units {int(u)} and {int(u) + 1} are neighbours' for u in (state[:-1] & state[1:]).nonzero().flatten()]
    for t0 in range(0, M, TILE):
        units = unit[t0:t0 + TILE]
        rows = clean_rows[t0:t0 + TILE]
        if int(units[0]) != int(units[-1]) and bool(rows.all()):
            gaps.append(f'tile at row {t0} holds units {int(units[0])} .. {int(units[-1])} and no poison')
    return gaps


# ---------------------------------------------------------------------------------------------------------------------- the comparison
def assert_clean_equal(got, want, clean, what=''):
    """THE comparison: the elements of `got` (poisoned neighbours) selected by `clean` equal those of `want` (the clean run of the same
    launch shape) bit for bit, and are finite.  clean: bool, [rows] or anything that broadcasts against got.reshape(rows, -1)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    clean = clean.to(got.device)
    if clean.dim() == 1:
        clean = clean[:, None]
    sel = clean.expand_as(g)
    a, b = g[sel], w[sel]
    if a.is_floating_point():
        assert bool(torch.isfinite(a).all()), f'{what}: {int((~torch.isfinite(a)).sum())} elements of clean units are not finite'
    diff = bits(a) != bits(b)
    assert not bool(diff.any()), f'{what}: {int(diff.sum())} of {diff.numel()} elements of clean units differ from the clean run'


def assert_poison_arrived(got, want, clean, what=''):
    """The poisoned units' outputs differ from the clean run's: the poison was where the kernel reads (a test that poisons bytes nobody
    reads would pass everything)."""
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    clean = clean.to(got.device)
    if clean.dim() == 1:
        clean = clean[:, None]
    sel = (~clean).expand_as(g)
    if bool(sel.any()):
        assert bool((bits(g[sel]) != bits(w[sel])).any()), f'{what}: the poisoned units came out as in the clean run'


# ---------------------------------------------------------------------------------------------------------------------- the plan
def _on(switches, name, dflt=True):
    """env_on of csrc/vit.hip: unset = the default, otherwise atoi(value) != 0."""
    if name not in switches:
        return dflt
    try:
        return int(switches[name]) != 0
    except ValueError:
        return False


def plan(cfg, n, dtype='f16', switches=None):
    """vit_resolve_switches + vit_plan restated: -> (stream form, cls_only_last) of an encode of n crops.
    stream form: 'f32' (separate LayerNorm launches), 'fold' (fp32 stream, LayerNorms folded into the GEMMs), 'pair' (fp16 pair),
    'f16' (VG_VIT_RESID16).  Two crop counts whose plans are equal run the same kernels on every row."""
    sw = switches or {}
    W, layers = cfg['width'], cfg.get('layers', 2)
    T = (cfg['resolution'] // cfg['patch']) ** 2 + 1
    f16 = dtype == 'f16'
    w4, cls_last = _on(sw, 'VG_GEMM_W4'), _on(sw, 'VG_VIT_CLS_LAST')
    resid_h = f16 and W % 256 == 0 and 'VG_VIT_RESID16' in sw
    fold = f16 and W % 256 == 0 and not resid_h and _on(sw, 'VG_VIT_LN_FOLD')
    resid_hl = fold and w4 and cls_last and W <= 1024 and _on(sw, 'VG_VIT_RESID_HL')
    Mp, Mc, es, stats = VS.pad256(n * T), VS.pad256(n), 2 if f16 else 4, (W // 64) * 8
    tail = Mc * (W * 4 + W * 2 + W * 2 + 4 * W * 2 + stats)
    query = Mc * (W * 2 + W * 2 + stats)
    fits = tail <= Mp * (3 * W + 256) * es and query <= Mp * 4 * W * es
    cls_only = cls_last and fold and layers > 1 and fits
    stream = 'f16' if resid_h else 'pair' if resid_hl and cls_only else 'fold' if fold else 'f32'
    return stream, cls_only


def workspace_bytes(cfg, n, dtype='f16', switches=None):
    """What vg_vit_workspace_bytes reports for the handle plan() describes (vit_stages_ref.region's closed form)."""
    sw = switches or {}
    fold = dtype == 'f16' and cfg['width'] % 256 == 0 and 'VG_VIT_RESID16' not in sw and _on(sw, 'VG_VIT_LN_FOLD')
    return VS.region(cfg, dtype, n, fold)['total']


def same_plan_counts(cfg, n, dtype='f16', switches=None):
    """Every m < n whose plan equals n's."""
    want = plan(cfg, n, dtype, switches)
    return [m for m in range(1, n) if plan(cfg, m, dtype, switches) == want]


# ---------------------------------------------------------------------------------------------------------------------- the graph cache
class LruModel:
    """The counters of vg_graph_cache behind ONE handle whose calls all share a launch form: the handle's first call (and the first after
    `invalidate`: a weight or the input norm was replaced, the derived tensors are rebuilt) runs as plain launches and counts nowhere;
    a key not in the cache is captured, after the least recently used graphs made room; every other call replays."""

    def __init__(self, limit):
        self.limit, self.warm, self.live = limit, False, []          # live: least recently used first
        self.captured = self.launches = self.evicted = 0

    def invalidate(self):
        self.warm = False

    def stats(self):
        return {'graphs_captured': self.captured, 'graph_launches': self.launches, 'graphs_evicted': self.evicted, 'graphs_live': len(self.live)}

    def step(self, key):
        if not self.warm:
            self.warm = True
            return self.stats()
        if key in self.live:
            self.live.remove(key)
        else:
            while len(self.live) >= self.limit:
                self.live.pop(0)
                self.evicted += 1
            self.captured += 1
        self.live.append(key)
        self.launches += 1
        return self.stats()
