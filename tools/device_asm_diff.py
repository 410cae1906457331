"""Is the device code of this tree the device code of another tree?  For refactors that must not touch a kernel.

    python tools/device_asm_diff.py <other-tree> [source ...]        # default: every .hip of build.SOURCES

Compiles csrc/<source> of both trees to device assembly with the product flags (build._device_asm) and compares the texts without
the lines that name the per-file symbol __hip_cuid_<hash>.  If they differ as a whole -- a kernel moved, say -- it compares kernel by
kernel: the same set of symbols, and per symbol the text from its label to its .Lfunc_end plus its .amdhsa_kernel block, with the
function's running number taken out of the local labels (.LBB<n>_<m>, .Lfunc_end<n>) and of the comments that cite them; and the
lines outside the function bodies (device globals, LDS symbols, sections, metadata) as a sorted list.
Prints a markdown report; exit 1 on a difference.
"""
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_of(tree):
    path = os.path.join(tree, 'vilgod_amd', 'build.py')
    spec = importlib.util.spec_from_file_location('vg_build_' + str(abs(hash(tree))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lines(text):
    return [l for l in text.splitlines() if '__hip_cuid_' not in l]


def _renumber(text):
    """local labels without the function's running number, comments without the padding that depends on a label's length"""
    text = re.sub(r'(\.L|\b)BB\d+_', r'\1BB_', text)
    text = re.sub(r'\.Lfunc_(end|begin)\d+', r'.Lfunc_\1', text)
    return re.sub(r'[ \t]+;', ' ;', text)


def kernels(text):
    """-> ({symbol: text of the function + its .amdhsa_kernel block}, the sorted lines outside the function bodies: globals, LDS
    symbols, sections, metadata), both renumbered"""
    out, rest = {}, []
    lines = _lines(text)
    i = 0
    while i < len(lines):
        m = re.match(r'^([A-Za-z_][\w$.]*):\s', lines[i] + ' ')
        if m and i > 0 and '@function' in lines[i - 1]:
            j = i
            while not lines[j].startswith('.Lfunc_end'):
                j += 1
            out[m.group(1)] = _renumber('\n'.join(lines[i:j + 1]))
            i = j
        else:
            rest.append(_renumber(lines[i]))
        i += 1
    for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', text, flags=re.M | re.S):
        out[m.group(1)] = out.get(m.group(1), '') + '\n' + m.group(2)
    return out, sorted(rest)


def compare(other_tree, source):
    """-> (lines, symbols compared, [what differs: symbols, or the text outside them], whole text equal)"""
    a = _build_of(os.path.abspath(other_tree))._device_asm(source)
    b = _build_of(ROOT)._device_asm(source)
    la, lb = _lines(a), _lines(b)
    (ka, ra), (kb, rb) = kernels(a), kernels(b)
    bad = sorted(set(ka) ^ set(kb)) + sorted(s for s in set(ka) & set(kb) if ka[s] != kb[s])
    if ra != rb:                                   # (as sorted lines: the metadata lists the kernels in the order they were emitted)
        bad.append('the text outside the kernels')
    return len(lb), len(kb), bad, la == lb


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sources = sys.argv[2:] or [s for s in _build_of(ROOT).SOURCES if s.endswith('.hip')]
    failed = False
    print('| source | assembly lines | symbols compared | whole text equal | symbols that differ |')
    print('|---|---|---|---|---|')
    for src in sources:
        n, nsym, bad, whole = compare(sys.argv[1], src)
        failed |= bool(bad)
        print(f'| `{src}` | {n} | {nsym} | {"yes" if whole else "no (kernel order)"} | {", ".join(bad) if bad else "none"} |')
    sys.exit(1 if failed else 0)
