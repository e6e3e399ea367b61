#!/usr/bin/env python3
"""Are two device-side assembly files of one unit the same code?

    hipcc $FLAGS [-DZK_FQU_INLINE for msm] --cuda-device-only -S -o old/zkhip.s zkhip.hip      (at the old commit)
    hipcc $FLAGS ...                       --cuda-device-only -S -o new/zkhip.s zkhip.hip      (at the new one)
    tools/device_asm_diff.py old/zkhip.s new/zkhip.s

A host-only change must leave every kernel as it was, instruction for instruction.  Two compilations of the same source differ in
the __hip_cuid_<hash> symbol only; a template kernel is emitted where host code first instantiates it, so moving a host function
reorders the functions of the file (and renumbers the BB<function>_<block> labels) without changing any of them.  This script
replaces the cuid, drops the function index from block labels, splits both files per function and per kernel-metadata entry, sorts
and compares: exit status 0 and "identical" twice, or the first differing functions and status 1."""
import re
import sys


def split(path):
    t = open(path).read()
    t = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', t)
    t = re.sub(r'BB\d+_', 'BB_', t)
    t = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', t)
    meta = t.index('\t.amdgpu_metadata') if '\t.amdgpu_metadata' in t else len(t)
    body, md = t[:meta], t[meta:]
    chunks = re.split(r'(?m)^(?=\t\.(?:section\t\.text|text|protected|globl|weak|rodata|section\t\.rodata)\b)', body)
    md = md.split('amdhsa.target')[0]                      # (the footer would stick to whichever kernel comes last)
    return sorted(c for c in chunks if c.strip()), sorted(re.split(r'(?m)^(?=  - \.)', md))


def main():
    a, am = split(sys.argv[1])
    b, bm = split(sys.argv[2])
    print('code chunks', len(a), len(b), 'identical' if a == b else 'DIFFERENT')
    print('metadata entries', len(am), len(bm), 'identical' if am == bm else 'DIFFERENT')
    for only, name in ((set(a) - set(b), 'first'), (set(b) - set(a), 'second')):
        for c in sorted(only)[:3]:
            print('only in the %s:\n%s' % (name, c[:600]))
    return 0 if a == b and am == bm else 1


if __name__ == '__main__':
    sys.exit(main())
