"""ctypes binding of libvilgod_hip.so.

The prototypes are parsed from include/vilgod_hip.h, so the header is the single source of truth
for the ABI.  There is NO fallback: if the library is missing or a symbol cannot be resolved the
import fails loudly (the hot path has no CPU implementation in this package).
"""
import ctypes
import os
import re

# torch ships its own libamdhip64; it must be in the process BEFORE our library is loaded so that both resolve to
# ONE HIP runtime (otherwise our hipMalloc lands in a second, uninitialised runtime: "no ROCm-capable device").
import torch  # noqa: F401  (plumbing: device memory, streams, torch.distributed)

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vilgod_hip.h')
LIB_PATH = os.environ.get('VILGOD_HIP_LIB') or os.path.join(HERE, 'libvilgod_hip.so')       # override: A/B runs of two builds on one box

_SCALARS = {
    'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
    'uint64_t': ctypes.c_uint64, 'uint8_t': ctypes.c_uint8, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
    'void': None,
}


class VilgodHipError(RuntimeError):
    pass


def parse_header(path=HEADER):
    """-> {name: (restype, [(ctype, argname), ...])} for every `vg_*` prototype."""
    src = open(path).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    src = re.sub(r'//[^\n]*', ' ', src)
    protos = {}
    for m in re.finditer(r'\b(int|void|int64_t|size_t|double|const\s+char\s*\*)\s+(vg_\w+)\s*\(([^)]*)\)\s*;', src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        sig = []
        if args and args != 'void':
            for a in args.split(','):
                a = ' '.join(a.split())
                if '*' in a:
                    sig.append((ctypes.c_void_p, a.split('*')[-1].strip()))
                else:
                    toks = a.replace('const ', '').split()
                    sig.append((_SCALARS[toks[0]], toks[-1]))
        if 'char' in ret:
            restype = ctypes.c_char_p
        else:
            restype = _SCALARS[ret]
        protos[name] = (restype, sig)
    return protos


def _load():
    if not os.path.exists(LIB_PATH):
        raise VilgodHipError(
            f'{LIB_PATH} not found. Build it first:  python -m vilgod_amd.build  '
            '(there is no CPU fallback for the hot path).')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, sig) in parse_header().items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise VilgodHipError(f'{LIB_PATH} does not export {name} declared in {HEADER}; rebuild') from e
        fn.restype = restype
        fn.argtypes = [t for t, _ in sig]
    return lib


lib = _load()

# the integer `#define VG_*` constants of the header, read once: a missing name is a KeyError at import (a define whose value is
# not a plain decimal integer -- 0.5, 0x10 -- is absent, never truncated)
_DEFINES = {m.group(1): int(m.group(2))
            for m in re.finditer(r'^#define[ \t]+VG_(\w+)[ \t]+(\d+)[ \t]*(?:/\*.*|//.*)?$', open(HEADER).read(), flags=re.M)}

# largest min_samples vg_cluster_mst[_nd] takes
CLUSTER_MAX_K = _DEFINES['CLUSTER_MAX_K']

# vg_cluster_filter_ex: column order of d_verdict / vg_filter_params.active (include/vilgod_hip.h VG_FILTER_*)
FILTER_NAMES = ('filter_by_number_points', 'filter_by_height', 'filter_by_aspect_ratio', 'filter_by_volume', 'filter_by_area',
                'filter_by_plane_distance', 'filter_by_ephemeral_score')
FILTER_AND_REQUIRED, FILTER_AND, FILTER_OR = (_DEFINES['FILTER_' + k] for k in ('AND_REQUIRED', 'AND', 'OR'))
FILTER_NSTATS = _DEFINES['FILTER_NSTATS']
FILTER_FLAG_DEGENERATE, FILTER_FLAG_HULL_OVERFLOW = _DEFINES['FILTER_FLAG_DEGENERATE'], _DEFINES['FILTER_FLAG_HULL_OVERFLOW']
BOX_MAX_HULL = _DEFINES['BOX_MAX_HULL']                   # vg_cluster_boxes d_aux3 (VG_BOX_*)
BOX_FLAG_DEGENERATE, BOX_FLAG_HULL_OVERFLOW = _DEFINES['BOX_FLAG_DEGENERATE'], _DEFINES['BOX_FLAG_HULL_OVERFLOW']


class FilterParams(ctypes.Structure):
    """vg_filter_params (include/vilgod_hip.h), passed by reference to vg_cluster_filter_ex."""
    _fields_ = [
        ('active', ctypes.c_int * 7), ('logic', ctypes.c_int * 7),
        ('min_points', ctypes.c_int), ('max_points', ctypes.c_int),
        ('has_max_volume', ctypes.c_int), ('has_max_area', ctypes.c_int),
        ('min_height', ctypes.c_double), ('max_height', ctypes.c_double),
        ('min_aspect_ratio', ctypes.c_double), ('max_aspect_ratio', ctypes.c_double),
        ('min_volume', ctypes.c_double), ('max_volume', ctypes.c_double),
        ('min_area', ctypes.c_double), ('max_area', ctypes.c_double),
        ('max_min_height', ctypes.c_double), ('min_max_height', ctypes.c_double),
        ('percentile', ctypes.c_double), ('min_percentile_pp_score', ctypes.c_double),
    ]

    def __init__(self):
        super().__init__()
        lib.vg_filter_default_params(ctypes.byref(self))


class RenderParams(ctypes.Structure):
    """vg_render_params (include/vilgod_hip.h), passed by reference to vg_render_crops_ex.  `one_plus_bias` is 1 + depth_bias formed in
    double and rounded to float32, which is what torch does with the Python scalar at mv_utils.py:110."""
    _fields_ = [('resolution', ctypes.c_int), ('depth', ctypes.c_int),
                ('obj_ratio', ctypes.c_float), ('depth_bias', ctypes.c_float), ('one_plus_bias', ctypes.c_float)]

    def __init__(self, resolution=112, depth=8, obj_ratio=0.8, depth_bias=0.2):
        super().__init__(int(resolution), int(depth), float(obj_ratio), float(depth_bias), 1.0 + float(depth_bias))


RENDER_RESOLUTION = (_DEFINES['RENDER_MIN_RESOLUTION'], _DEFINES['RENDER_MAX_RESOLUTION'])
RENDER_DEPTH = (_DEFINES['RENDER_MIN_DEPTH'], _DEFINES['RENDER_MAX_DEPTH'])
PREPROCESS_IMAGE_SIZE = (_DEFINES['PREPROCESS_MIN_IMAGE_SIZE'], _DEFINES['PREPROCESS_MAX_IMAGE_SIZE'])     # vg_clip_preprocess


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def check(status, what=''):
    if status != 0:
        names = {1: 'bad argument', 2: 'HIP runtime error', 3: 'capacity exceeded'}
        raise VilgodHipError(f'{what} failed: status {status} ({names.get(status, "?")})')
