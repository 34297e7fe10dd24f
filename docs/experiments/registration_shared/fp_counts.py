#!/usr/bin/env python3
"""Floating-point instructions per kernel of two builds, side by side (parent / new), from the assembly that
docs/experiments/conv_ep_bf16/compare_kernels.py compares:
    python fp_counts.py PARENT_DIR NEW_DIR NAME ...
A line per kernel whose counts differ, then one line with the number of kernels whose counts agree."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'conv_ep_bf16'))
from compare_kernels import kernels, short  # noqa: E402

FP = re.compile(r'^(v_(fma|fmac|mul|add|sub|mad|mac|rcp|rsq|sqrt|div_\w+|trig\w*|ldexp|frexp\w*|floor|ceil|fract|rndne|trunc|min|max|cvt)'
                r'\w*_(f32|f64)\w*|v_cvt_\w+|v_pk_\w+_f32)\b')


def counts(body):
    c = collections.Counter()
    for line in body:
        m = FP.match(line)
        if m:
            c[line.split()[0]] += 1
    return c


parent, new, names = sys.argv[1], sys.argv[2], sys.argv[3:]
same = 0
for n in names:
    kp, kn = kernels('%s/%s.s' % (parent, n)), kernels('%s/%s.s' % (new, n))
    for k in sorted(set(kp) & set(kn)):
        cp, cn = counts(kp[k]), counts(kn[k])
        if cp == cn:
            same += 1
            print('%s: %d floating-point instructions, the same in both builds' % (short(k), sum(cp.values())))
            continue
        print('%s: %s' % (short(k), ', '.join('%s %d / %d' % (op, cp[op], cn[op]) for op in sorted(set(cp) | set(cn)) if cp[op] != cn[op])))
print('%d kernels with the same counts' % same)
