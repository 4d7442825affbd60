#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files of the same source, for changes that must leave the device code alone
(host-side refactors, removed preprocessor branches).  Build both with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fuse-cuid=none -x hip -S --cuda-device-only FILE.hip -o FILE.s
and run   tools/isa_diff.py OLD.s NEW.s [OLD2.s NEW2.s ...].  Compared per .amdhsa_kernel symbol, not as whole files (the order of
instantiation may differ): the instruction text, the .amdhsa_ descriptor block and the metadata entry.  Three things are normalised:
the per-compile __hip_cuid_<hex> symbol, the function ordinal in local labels (.LBB<n>_<k>, .Lfunc_end<n>, and BB<n>_<k> in comments)
and the blanks in front of a comment (the column padding behind a label depends on the ordinal's digit count).  Exit status 1 when a
kernel is missing on either side or differs.
With --opcodes in front, every kernel that differs also gets a line for changes that may re-order a kernel but must keep its
instructions (a helper function taken out of it): instructions before -> after, the opcodes whose COUNT moved (_e32 / _e64 encodings
of one opcode counted together), VGPRs, static LDS bytes and scratch bytes before -> after."""
import collections
import re
import sys


def kernels(path):
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid', open(path).read())
    text = re.sub(r'\.L([A-Za-z_]+?)\d+(_\d+)?\b', r'.L\1#\2', text)
    text = re.sub(r'\bBB\d+_(\d+)\b', r'BB#_\1', text)   # the same labels inside the compiler's comments ("Loop: Header=BB28_3")
    text = re.sub(r'[ \t]+;', ' ;', text)                # comments are padded to a column: an ordinal of 9 -> 10 moves the padding behind its labels
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.M | re.S):
        name = m.group(1)
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end#:' % re.escape(name), text, re.M | re.S).group(1)   # (holds the descriptor too)
        out[name] = {'code': body.replace(m.group(2), ''), 'descriptor': m.group(2)}
    meta = text.split('amdhsa.kernels:')[1].split('amdhsa.target:')[0]
    for blk in re.split(r'^  - ', meta, flags=re.M)[1:]:
        out[re.search(r'\.name:\s+(\S+)', blk).group(1)]['metadata'] = blk
    return out


def opcodes(code):
    c = collections.Counter()
    for line in code.split('\n'):
        line = line.split(';')[0].strip()
        if line and not line.startswith('.') and not line.endswith(':'):
            c[re.sub(r'_e(32|64)$', '', line.split()[0])] += 1
    return c


def resources(k):
    field = lambda text, name: int(re.search(r'%s:?\s+(\d+)' % re.escape(name), text).group(1))   # noqa: E731
    return (field(k['descriptor'], '.amdhsa_next_free_vgpr'), field(k['metadata'], '.group_segment_fixed_size'),
            field(k['metadata'], '.private_segment_fixed_size'))


def opcode_line(a, b):
    oa, ob = opcodes(a['code']), opcodes(b['code'])
    moved = ', '.join(f'{o} {oa[o]} -> {ob[o]}' for o in sorted(set(oa) | set(ob)) if oa[o] != ob[o]) or 'none'
    (va, la, sa), (vb, lb, sb) = resources(a), resources(b)
    return (f'    instructions {sum(oa.values())} -> {sum(ob.values())}; opcode counts moved: {moved}; VGPRs {va} -> {vb}, LDS {la} -> {lb}, '
            f'scratch {sa} -> {sb}')


def main(argv):
    bad = 0
    with_opcodes = argv[:1] == ['--opcodes']
    argv = argv[1:] if with_opcodes else argv
    for old, new in zip(argv[0::2], argv[1::2]):
        a, b = kernels(old), kernels(new)
        differ = [(k, [p for p in a[k] if a[k][p] != b[k].get(p)]) for k in sorted(set(a) & set(b)) if a[k] != b[k]]
        for k in sorted(set(a) ^ set(b)):
            print(f'  only in {old if k in a else new}: {k}')
        for k, parts in differ:
            print(f'  differs ({", ".join(parts)}): {k}')
            if with_opcodes:
                print(opcode_line(a[k], b[k]))
        print(f'{new}: {len(a)} kernels before, {len(b)} after, {len(differ)} of {len(set(a) & set(b))} differ')
        bad += len(differ) + len(set(a) ^ set(b))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
