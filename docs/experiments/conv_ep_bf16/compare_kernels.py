"""Kernel-by-kernel comparison of two builds of some sources (by default the bf16 convolution sources).

For each source both builds are compiled to gfx950 assembly with the resource remarks on stderr:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-sched-strategy=max-ilp --cuda-device-only -S \
          -Rpass-analysis=kernel-resource-usage csrc/NAME.hip -o DIR/NAME.s 2> DIR/NAME.remarks

(the flags of csrc/build.sh for these sources).  This script then compares the instruction stream of every kernel symbol
-- comments, directives outside the body and the numbering of local labels dropped -- and, for the kernels that differ,
prints a table of the resources of both builds side by side (parent / new).

    python compare_kernels.py [--map MAP.json] PARENT_DIR NEW_DIR [NAME ...]

NAME ...: the sources to compare (without .hip).  MAP.json: {parent symbol: new symbol, or null for a kernel deleted on purpose},
for kernels whose mangled names changed; a deleted kernel is listed and left out of the comparison.

Exit status 1 if a kernel gained scratch bytes or lost an occupancy step, or if the two builds do not hold the same kernels."""
import json
import re
import sys

NAMES = ['convp_bf16', 'convq_bf16', 'convn_bf16', 'convs', 'wgradp_bf16']
KEYS = ['VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]']


def kernels(path):
    """symbol -> list of normalised instruction lines"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r'^\.Lfunc_end\d+:', line):
            out[name] = cur
            cur = None
            continue
        line = line.split(';')[0].strip()
        if not line or line.startswith(('.loc', '.file', '.cfi', '.p2align')):
            continue
        cur.append(re.sub(r'\.L(BB|tmp|func_\w+?)\d+(_\d+)?', lambda g: '.L' + g.group(1) + (g.group(2) or ''), line))
    return out


def short(sym):
    """_ZN3dfl...12convq_kernelILi128ELi1E...EEvNS_5ConvPE -> convq_kernel<128,1,...>"""
    for m in re.finditer(r'(\d+)(?=([a-z][a-z0-9_]*_kernel)(I\S*)?)', sym):    # <length><name>: rs_u8_kernel has a digit of its own
        if int(m.group(1)) == len(m.group(2)):
            lits = re.findall(r'L[ib](\d+)E', m.group(3) or '')    # every literal template argument, nested ones included
            return m.group(2) + ('<%s>' % ','.join(lits) if lits else '')
    return sym


def renamed(table, mapping, body=False):
    """the parent's table under the new build's symbol names; kernels mapped to null are dropped"""
    out = {}
    for k, v in table.items():
        if k in mapping and mapping[k] is None:
            continue
        if body:
            for old, new in mapping.items():
                if new is not None:
                    v = [line.replace(old, new) for line in v]
        out[mapping.get(k, k)] = v
    return out


def resources(path):
    """symbol -> {resource: value} from the kernel-resource-usage remarks"""
    out, name = {}, None
    for line in open(path):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass', line)
        if m and name is not None:
            out[name][m.group(1)] = m.group(2)
    return out


def main():
    argv, mapping = sys.argv[1:], {}
    if argv[0] == '--map':
        mapping, argv = json.load(open(argv[1])), argv[2:]
    parent, new = argv[0], argv[1]
    names = argv[2:] or NAMES
    bad = False
    for n in names:
        kp, kn = kernels('%s/%s.s' % (parent, n)), kernels('%s/%s.s' % (new, n))
        rp, rn = resources('%s/%s.remarks' % (parent, n)), resources('%s/%s.remarks' % (new, n))
        for k in sorted(k for k in rp if k in mapping and mapping[k] is None):
            print('%s: deleted on purpose: %s (%s VGPRs)' % (n, k, rp[k].get('VGPRs')))
        kp, rp = renamed(kp, mapping, body=True), renamed(rp, mapping)
        glob_p = sorted(k for k in kp if k in rp)
        glob_n = sorted(k for k in kn if k in rn)
        if glob_p != glob_n:
            bad = True
            print('%s: kernel sets differ: only parent %s, only new %s' % (n, sorted(set(glob_p) - set(glob_n)), sorted(set(glob_n) - set(glob_p))))
        both = [k for k in glob_p if k in kn]
        diff = [k for k in both if kp[k] != kn[k]]
        print('%s: %d kernels, %d identical, %d differ' % (n, len(both), len(both) - len(diff), len(diff)))
        for k in both:
            sp, sn = int(rp[k]['ScratchSize [bytes/lane]']), int(rn[k]['ScratchSize [bytes/lane]'])
            op, on = int(rp[k]['Occupancy [waves/SIMD]']), int(rn[k]['Occupancy [waves/SIMD]'])
            if sn > sp or on < op:
                bad = True
                print('  WORSE %s: scratch %d -> %d, occupancy %d -> %d' % (k, sp, sn, op, on))
        if diff:
            print('\n| kernel | instructions | VGPRs | AGPRs | SGPRs | scratch B/lane | static LDS B | waves/SIMD |\n|---|---|---|---|---|---|---|---|')
        for k in diff:
            print('| `%s` | %d / %d | %s |' % (short(k), len(kp[k]), len(kn[k]), ' | '.join('%s / %s' % (rp[k].get(key), rn[k].get(key)) for key in KEYS)))
        if diff:
            print()
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
