#!/usr/bin/env python
"""Compare the register / LDS / scratch figures of every kernel in two sets of gfx950 assembly files.

    codegen_compare.py OLD_DIR NEW_DIR [--out TABLE.txt]

Both directories hold `hipcc -S --cuda-device-only` output of the same sources (one NAME.s per translation unit, the way
tests/test_isa_guard.py compiles them).  For every kernel of OLD the figures of the code-object metadata (.vgpr_count,
.sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size) must be the same in NEW; kernels only NEW has are
listed as added.  Kernels are matched by demangled name; a kernel of NEW whose template argument list is OLD's plus one
trailing `false` (a compile-time switch added with its default) counts as the same kernel.  Exit status 1 when a kernel of OLD is
missing from NEW or differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys

CXXFILT = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'


def demangle(names):
    out = subprocess.run([CXXFILT], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return [re.sub(r'^void ', '', d).replace('(anonymous namespace)::', '') for d in out[:len(names)]]


def keys_of(name):
    """The names under which a kernel of NEW answers: its own, and the one without a trailing `false` template argument."""
    head, sep, tail = name.partition('(')
    keys = [name]
    if head.endswith(', false>'):
        keys.append(head[:-len(', false>')] + '>' + sep + tail)
    elif head.endswith('<false>'):
        keys.append(head[:-len('<false>')] + sep + tail)
    return keys

KEYS = ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def kernels(path):
    """{kernel symbol: (vgpr, sgpr, lds, scratch)} from the amdhsa.kernels metadata of one .s file."""
    txt = open(path).read()
    meta = txt[txt.rfind('amdhsa.kernels:'):]
    out = {}
    for entry in re.split(r'\n  - \.a', meta)[1:]:
        entry = '.a' + entry
        name = re.search(r'^\s+\.name:\s+(\S+)', entry, re.M).group(1)
        out[name] = tuple(int(re.search(rf'^\s+\{k}:\s+(\d+)', entry, re.M).group(1)) for k in KEYS)
    names = sorted(out)
    return {d: out[n] for n, d in zip(names, demangle(names))} if names else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--out')
    a = ap.parse_args()
    lines, bad = [f'{"unit":18s} {"kernel":100s} {"vgpr":>5s} {"sgpr":>5s} {"lds":>7s} {"scratch":>7s}  status'], 0
    for f in sorted(os.listdir(a.old)):
        if not f.endswith('.s'):
            continue
        old, new_raw = kernels(os.path.join(a.old, f)), kernels(os.path.join(a.new, f))
        new, matched = {}, set()
        for n, v in new_raw.items():
            for key in keys_of(n):
                new.setdefault(key, (n, v))
        for k in sorted(old):
            if k not in new:
                status, bad = 'MISSING', bad + 1
            else:
                matched.add(new[k][0])
                if new[k][1] != old[k]:
                    status, bad = 'CHANGED -> ' + ' '.join(map(str, new[k][1])), bad + 1
                else:
                    status = 'same'
            lines.append(f'{f[:-2]:18s} {k[:100]:100s} {old[k][0]:5d} {old[k][1]:5d} {old[k][2]:7d} {old[k][3]:7d}  {status}')
        for k in sorted(set(new_raw) - matched):
            v = new_raw[k]
            lines.append(f'{f[:-2]:18s} {k[:100]:100s} {v[0]:5d} {v[1]:5d} {v[2]:7d} {v[3]:7d}  added')
    lines.append(f'{bad} kernel(s) of the old set missing or changed')
    text = '\n'.join(lines) + '\n'
    if a.out:
        open(a.out, 'w').write(text)
    sys.stdout.write(text if bad else lines[-1] + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
