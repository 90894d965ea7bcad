#!/usr/bin/env python3
"""Compare the device functions of two builds, from their gfx950 assembly (hipcc ... --offload-device-only -S x.hip -o x.s):
    tools/compare_kernels.py before.s after.s [before2.s after2.s ...]
Keyed by mangled symbol: the set of symbols, each kernel's descriptor (.amdhsa_kernel block: registers, scratch, LDS, wavefront
size) and each function's instruction stream after dropping comments and renumbering local labels.  Prints one line per pair
of files and every symbol that differs; exit status 1 if anything does.

    tools/compare_kernels.py --by-content before.s [before2.s ...] -- after.s [after2.s ...]
For builds whose kernel SYMBOLS differ (a renamed or re-parameterised kernel template, kernels moved to other files): each side is
the union of its files; kernels are matched by content -- the multiset of (descriptor, instruction stream), a kernel's own mangled
name replaced by a placeholder in both -- and every other device function by (symbol, instruction stream), once however many
files carry a copy.  Prints what is left unmatched on either side and one summary line; exit status 1 if anything is."""
import collections
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


def by_content(paths):
    """(Counter of kernels as (descriptor, instructions) -> [symbols], set of the other functions as (symbol, instructions))"""
    kernels, others = collections.defaultdict(list), set()
    for path in paths:
        body, desc = functions(path)
        for name, lines in body.items():
            if name in desc:
                own = lambda rows: tuple(row.replace(name, '<self>') for row in rows)
                kernels[(own(desc[name]), own(lines))].append(name)
            else:
                others.add((name, tuple(lines)))
    return kernels, others


def main_by_content(argv):
    if '--' not in argv or not argv[:argv.index('--')] or not argv[argv.index('--') + 1:]:
        print(__doc__)
        return 2
    (k0, f0), (k1, f1) = by_content(argv[:argv.index('--')]), by_content(argv[argv.index('--') + 1:])
    left = 0
    for side, mine, theirs in (('before', k0, k1), ('after', k1, k0)):
        for key, names in sorted(mine.items(), key=lambda item: item[1]):
            for name in names[len(theirs.get(key, ())):]:
                left += 1
                print(f'  unmatched kernel, {side} only ({len(key[1])} instructions): {name}')
                for other in theirs:                                       # the same instructions under another descriptor: show the fields
                    if other[1] == key[1]:
                        for line in sorted(set(key[0]) ^ set(other[0])):
                            print(f'      {line}')
                        break
    for side, mine, theirs in (('before', f0, f1), ('after', f1, f0)):
        for name, lines in sorted(mine - theirs):
            left += 1
            print(f'  unmatched function, {side} only ({len(lines)} instructions): {name}')
    count = lambda kernels: sum(len(names) for names in kernels.values())
    print(f'by content: {count(k0)} kernels / {len(f0)} other functions before, {count(k1)} / {len(f1)} after, {left} unmatched')
    return 1 if left else 0


def main(argv):
    if argv[:1] == ['--by-content']:
        return main_by_content(argv[1:])
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
