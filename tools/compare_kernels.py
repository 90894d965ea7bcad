#!/usr/bin/env python3
"""Compare the device functions of two builds, from their gfx950 assembly (hipcc ... --offload-device-only -S x.hip -o x.s):
    tools/compare_kernels.py before.s after.s [before2.s after2.s ...]
Keyed by mangled symbol: the set of symbols, each kernel's descriptor (.amdhsa_kernel block: registers, scratch, LDS, wavefront
size) and each function's instruction stream after dropping comments and renumbering local labels.  Prints one line per pair
of files and every symbol that differs; exit status 1 if anything does."""
import re
import sys


def functions(path):
    """{symbol: (instruction lines, descriptor lines)}"""
    body, desc = {}, {}
    name = kernel = None
    for raw in open(path):
        line = raw.split(';', 1)[0].strip()
        if not line:
            continue
        m = re.match(r'\.amdhsa_kernel\s+(\S+)', line)                    # (the descriptor sits in front of the function's end label)
        if m:
            kernel = m.group(1)
            desc[kernel] = []
        elif line == '.end_amdhsa_kernel':
            kernel = None
        elif kernel is not None:
            desc[kernel].append(line)
        elif re.match(r'\.type\s+(\S+),@function', line):
            name = re.match(r'\.type\s+(\S+),@function', line).group(1)
            body[name] = []
        elif name is not None:
            if re.match(r'\.Lfunc_end\d+:', line):
                name = None
            elif line != name + ':' and not line.startswith(('.p2align', '.globl', '.weak', '.protected', '.hidden', '.section', '.text')):
                body[name].append(re.sub(r'\.L(BB|tmp|func_begin|post_getpc)\d+(_\d+)?', lambda t: '.L' + t.group(1) + (t.group(2) or ''), line))
    return body, desc


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        print(__doc__)
        return 2
    bad = 0
    for before, after in zip(argv[0::2], argv[1::2]):
        (b0, d0), (b1, d1) = functions(before), functions(after)
        differ = sorted(set(b0) ^ set(b1) | set(d0) ^ set(d1))
        for s in differ:
            print(f'  only in one build: {s}')
        for s in sorted(set(b0) & set(b1)):
            what = [w for w, x, y in (('instructions', b0[s], b1[s]), ('descriptor', d0.get(s), d1.get(s))) if x != y]
            if what:
                differ.append(s)
                print(f'  differs ({", ".join(what)}): {s}')
                for line in sorted(set(d0.get(s) or []) ^ set(d1.get(s) or [])):
                    print(f'      {line}')
        print(f'{before} | {after}: {len(d0)} kernels / {len(b0)} functions before, {len(d1)} / {len(b1)} after, {len(differ)} differ')
        bad += len(differ)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
