"""Route identity of two builds of libdfl_hip.so on the host queries (no GPU needed):

    python docs/experiments/convs_unified/route_sweep.py PARENT_LIB NEW_LIB > docs/experiments/convs_unified/route_sweep.txt

Each library is loaded through DFL_LIB_OVERRIDE in a child process of its own, once as it stands and once under DFL_CONVS=0.  A
child answers, in the three arithmetics, for every block of cases.py, every convolution block of the eval-mode paper plan at
192 x 192 and 96 x 96 (batch 1) and, for each of those, the variants that must NOT take the latency form (statistics pointers,
x_mode, out_scale with accumulate, the 1.5 GFLOP cap):
    dfl_conv_config, dfl_conv_suggest_splits, dfl_conv_config with splits forced to 1, 2, 4 and 16, dfl_conv_pair_ok.
Every answer must be identical; the exit code says so."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402

LATENCY = 16 + 39


def child():
    sys.path.insert(0, cases.ROOT)
    import torch
    import dfl_amd
    from dfl_amd import _native as nat
    lib = nat.lib()
    rows = []
    nxt = [1 << 32]

    def alloc(name, count, kind):
        nxt[0] += (count * 4 + 4095) // 256 * 256
        return nxt[0]

    def ask(a):
        q = cases.copy_args(nat, a)
        ans = [lib.dfl_conv_config(C.addressof(q)), lib.dfl_conv_suggest_splits(C.addressof(q))]
        for sp in (1, 2, 4, 16):
            q = cases.copy_args(nat, a)
            q.splits, q.partial = sp, alloc('partial', 1 << 20, 'f32')
            ans.append(lib.dfl_conv_config(C.addressof(q)))
        return ans

    def variants(a):
        yield 'base', a
        q = cases.copy_args(nat, a)
        q.stat_partials = alloc('stats', 1 << 16, 'f32')
        yield 'stat_partials', q
        q = cases.copy_args(nat, a)
        q.stat_totals = alloc('totals', 1 << 16, 'f32')
        yield 'stat_totals', q
        q = cases.copy_args(nat, a)
        q.x_mode, q.x2, q.ldx2 = 1, alloc('x2', 1 << 20, 'act'), q.ldx
        q.in_scale = q.in_shift = None               # (a well-formed x_mode block without coefficients: what refuses it is x_mode itself)
        yield 'x_mode', q
        q = cases.copy_args(nat, a)
        q.out_scale, q.out_shift, q.accumulate = alloc('osc', 4096, 'f32'), alloc('osh', 4096, 'f32'), 1
        yield 'out_scale+accumulate', q
        q = cases.copy_args(nat, a)                  # the 1.5 GFLOP cap: more images of the same layer
        flop = 2.0 * q.N * (q.Hin * q.Win if q.scatter2x2 else q.Hout * q.Wout) * q.Ntot * q.KH * q.KW * q.Cin
        q.N = q.N * (int(1.6e9 / flop) + 1)
        yield 'gflop_cap', q

    def sweep(mode, name, a, b=None):
        for vname, q in variants(a):
            row = dict(mode=mode, block=name, variant=vname, ans=ask(q))
            if b is not None:
                row['pair_ok'] = [lib.dfl_conv_pair_ok(C.addressof(q), C.addressof(b))]
                for sp in (2, 4):                    # ... and with K slices asked for
                    qq = cases.copy_args(nat, q)
                    qq.splits, qq.partial = sp, alloc('partial', 1 << 20, 'f32')
                    row['pair_ok'].append(lib.dfl_conv_pair_ok(C.addressof(qq), C.addressof(b)))
            rows.append(row)

    for mode, mm in cases.MODES.items():
        nat.check(lib.dfl_set_math_mode(mm), 'dfl_set_math_mode')
        for i, d in enumerate(cases.specs(mode)):
            a = cases.build(nat, mode, d['a'], alloc, 'c%d.a' % i)
            b = None
            if 'b' in d:
                b = cases.build(nat, mode, d['b'], alloc, 'c%d.b' % i)
                cases.pair_link(a, b, alloc, 'c%d' % i)
            sweep(mode, d['name'], a, b)
            if b is not None:
                sweep(mode, d['name'] + ' (second)', b)
        for size in (192, 96):
            convs, pairs, keep = cases.paper_blocks(nat, dfl_amd, torch, size, torch.device('cpu'))
            first = {C.addressof(a): b for a, b in pairs}
            for i, st in enumerate(convs):
                name = 'paper%d #%d %dx%d Cin%d N%d k%d s%d%s' % (size, i, st.Hin, st.Win, st.Cin, st.Ntot, st.KH, st.stride, ' scatter' if st.scatter2x2 else '')
                sweep(mode, name, st, first.get(C.addressof(st)))
    nat.check(lib.dfl_set_math_mode(0), 'dfl_set_math_mode')
    json.dump(rows, sys.stdout)


def run(libpath, convs):
    env = dict(os.environ, DFL_LIB_OVERRIDE=os.path.abspath(libpath))
    env.pop('DFL_CONVS', None)
    if convs is not None:
        env['DFL_CONVS'] = convs
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, check=True, stdout=subprocess.PIPE).stdout
    return json.loads(out)


def main():
    parent, new = sys.argv[1], sys.argv[2]
    bad = 0
    for convs in (None, '0'):
        rp, rn = run(parent, convs), run(new, convs)
        assert [(r['mode'], r['block'], r['variant']) for r in rp] == [(r['mode'], r['block'], r['variant']) for r in rn]
        print('== DFL_CONVS %s: %d argument blocks, %d answers each side, sha256 of the answers parent %s new %s' % (
            'unset' if convs is None else convs, len(rp), sum(len(r['ans']) + len(r.get('pair_ok', [])) for r in rp),
            hashlib.sha256(json.dumps(rp).encode()).hexdigest()[:16], hashlib.sha256(json.dumps(rn).encode()).hexdigest()[:16]))
        for mode in cases.MODES:
            for variant in ('base', 'stat_partials', 'stat_totals', 'x_mode', 'out_scale+accumulate', 'gflop_cap'):
                sel = [(a, b) for a, b in zip(rp, rn) if a['mode'] == mode and a['variant'] == variant]
                diff = [(a, b) for a, b in sel if a != b]
                lat = sum(1 for a, _ in sel if a['ans'][0] == LATENCY)
                sliced = sum(1 for a, _ in sel if a['ans'][0] == LATENCY and a['ans'][1] > 1)
                pairs = sum(1 for a, _ in sel if a.get('pair_ok', [0])[0] > 0)
                errs = sum(1 for a, _ in sel if a['ans'][0] < 0)
                print('%-7s %-21s blocks %4d  latency form %4d (K-sliced %3d)  pairs %3d  refused %3d  differing %d' % (
                    mode, variant, len(sel), lat, sliced, pairs, errs, len(diff)))
                for a, b in diff[:5]:
                    print('   DIFFERS', a, b)
                bad += len(diff)
    print('RESULT: %s' % ('identical' if bad == 0 else '%d differing blocks' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child()
    else:
        sys.exit(main())
