"""The C-ABI library loads on a CPU-only host and exports every symbol include/*.h declares.
No compute is called here (no GPU)."""
import ctypes
import glob
import os
import re

from conftest import ROOT


def test_every_declared_symbol_is_exported():
    from vilgod_amd import _lib
    declared = set()
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        declared |= set(_lib.parse_header(h).keys())
    assert len(declared) >= 5
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    assert _lib.lib.vg_abi_version() >= 1


def test_header_has_no_torch_types():
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        src = open(h).read()
        assert 'torch' not in re.sub(r'/\*.*?\*/', '', src, flags=re.S)
        assert 'at::' not in src and 'c10::' not in src


def test_header_cites_reference_lines():
    src = open(os.path.join(ROOT, 'include', 'vilgod_hip.h')).read()
    assert len(re.findall(r'\.(py|cpp|h):\d+', src)) >= 8


def test_cluster_kernels_hold_no_unencodable_64bit_literals():
    """ROCm 7.2's gfx950 back end can materialise a wave-uniform `double x = INFINITY` as `s_mov_b64 s[..], 0x7ff0000000000000`,
    which gfx9 cannot encode (the object file then holds 0.0; round 3, k_cl_core_far).  csrc/cluster.hip keeps such values in
    SGPRs, so its assembly is scanned here; `python -m vilgod_amd.build --check-isa` scans every source (vit.hip takes a minute)."""
    from vilgod_amd import build
    assert build.check_isa(sources=['cluster.hip']) == []


def test_vit_kernels_do_not_spill():
    """No kernel of csrc/vit.hip in the product library uses scratch memory: every instantiation of the projection GEMMs fits its
    256-register budget, and so do the attention kernels (round 3: an experimental persistent GEMM instantiation that spilled eight
    registers returned wrong values for the rows of one accumulator register -- spills in this file are treated as build errors
    since; the guard covered k_gemm_f16_pp64 only and the TR attention instantiation spilled a 64-bit row index unnoticed)."""
    from vilgod_amd import build
    assert build.check_scratch('vit.hip', '') == []


def test_w4_loop_is_what_its_generator_writes():
    """csrc/gemm_w4_loop.inc (the K loop of k_gemm_f16_w4: ~1 260 scheduled instructions per block) is generated; the committed file
    is what csrc/gen_gemm_w4.py emits."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'vilgod_amd', 'csrc', 'gen_gemm_w4.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_w4_epilogues_match_the_wait_counts_of_the_assembly_block():
    """The assembly block of k_gemm_f16_w4 waits for the NEXT tile's first DMA pieces with `vmcnt(24 + S)` / `vmcnt(8 + S)`, S = the
    stores the compiler-generated epilogue issues behind them (in-order retirement; gen_gemm_w4.py ST).  A smaller S in the binary than
    the generator assumed would let a fragment read run ahead of its piece.  Checked per instantiation, with: no scratch, and no
    compiler-inserted `vmcnt(0)` inside the tile loop (one that waits for a spill reload or a branched load drains the previous tile's
    stores: the first-tile set-up in front of the loop and the final drain behind it are the only ones)."""
    from vilgod_amd import build
    src = open(os.path.join(ROOT, 'vilgod_amd', 'csrc', 'gemm_w4_loop.inc')).read()
    st_h = int(re.search(r'#define VG_W4_STORES_H (\d+)', src).group(1))
    st_f = int(re.search(r'#define VG_W4_STORES_F (\d+)', src).group(1))
    res = build.check_w4_epilogues()
    assert set(res) == {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2), (3, 0), (5, 2)}, sorted(res)       # (5, 2): the residual stream as an fp16 pair
    for (epi, ln), r in res.items():
        assert r['scratch'] == 0, (epi, ln, r)
        if epi in (0, 1):
            assert r['stores'] == st_h, (epi, ln, r)        # exact: the allowance is 24 + S <= 63
        else:
            assert r['stores'] >= st_f, (epi, ln, r)        # the allowance is capped at the counter's 63
        zeros = [i for i, w in enumerate(r['compiler_vmcnt']) if w == 0]
        assert len(zeros) <= 2 and (not zeros or zeros[-1] == len(r['compiler_vmcnt']) - 1), (epi, ln, r['compiler_vmcnt'])


def _vit_product_text():
    """{file: text without comments} of csrc/vit.hip and the includes of csrc/ it pulls in, the development build's (csrc/dev/, the
    build's object directories) left out"""
    csrc = os.path.join(ROOT, 'vilgod_amd', 'csrc')
    texts, todo = {}, ['vit.hip']
    while todo:
        name = todo.pop()
        if name in texts or name.startswith('dev/') or not os.path.exists(os.path.join(csrc, name)):
            continue
        src = open(os.path.join(csrc, name)).read()
        todo += re.findall(r'^#include "([^"]+)"', src, flags=re.M)
        texts[name] = re.sub(r'//[^\n]*|/\*.*?\*/', lambda m: re.sub(r'[^\n]', ' ', m.group(0)), src, flags=re.S)
    return texts


def test_vit_reads_the_environment_in_one_place():
    """The product text of the ViT translation unit calls getenv only inside VitSwitches::from_env and the two env_* helpers it uses:
    a handle reads its switches once (vg_vit_create), the handle-less entry points once per call."""
    texts = _vit_product_text()
    assert {'vit.hip', 'vit_gemm_kernels.inc', 'vit_gemm_launch.inc', 'vit_attention.inc', 'gemm_w4_loop.inc'} <= set(texts), sorted(texts)
    stray = []
    for name, src in texts.items():
        allowed = []
        for m in re.finditer(r'static VitSwitches from_env\(\) \{|^static (?:int env_int|bool env_on)\([^\n]*\{', src, flags=re.M):
            depth, i = 1, m.end()
            while depth:
                depth += {'{': 1, '}': -1}.get(src[i], 0)
                i += 1
            allowed.append((m.start(), i))
        for m in re.finditer(r'\bgetenv\b', src):
            if not any(a <= m.start() < b for a, b in allowed):
                stray.append((name, src.count('\n', 0, m.start()) + 1))
    assert not stray, stray
    helpers = [n for n in texts if 'static VitSwitches from_env()' in texts[n]]
    assert helpers == ['vit.hip'], helpers
