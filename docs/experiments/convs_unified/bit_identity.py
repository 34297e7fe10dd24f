"""Bit identity of two builds of libdfl_hip.so on the latency form, on an MI355X:

    python docs/experiments/convs_unified/bit_identity.py PARENT_LIB NEW_LIB

Each library runs in a fresh child process (DFL_LIB_OVERRIDE).  A child runs, in the three arithmetics, every block of cases.py
on seeded operands through dfl_conv2d / dfl_conv2d_pair with the K slices the library suggests, and the eval-mode paper forward at
192 x 192, batch 1; it prints one SHA-256 per output tensor (raw bytes).  The parent process compares the two lists."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(__import__('torch').uint8).numpy().tobytes()).hexdigest()


def child():
    sys.path.insert(0, cases.ROOT)
    import torch
    import dfl_amd
    import bench
    from dfl_amd import _native as nat
    lib = nat.lib()
    DEV = 'cuda'
    rows = []
    st = lambda: torch.cuda.current_stream().cuda_stream

    for mode, mm in cases.MODES.items():
        nat.check(lib.dfl_set_math_mode(mm), 'dfl_set_math_mode')
        act = torch.bfloat16 if mode == 'bf16s' else torch.float32
        for i, d in enumerate(cases.specs(mode)):
            g = torch.Generator().manual_seed(1000 + i)
            keep = {}

            def alloc(name, count, kind):
                if kind == 'w_bf16':
                    t = (torch.randn(count // 2, generator=g) * 0.05).to(torch.bfloat16)
                elif kind == 'w_f32':
                    t = torch.randn(count // 4, generator=g) * 0.05
                elif kind == 'scale':
                    t = torch.rand(count, generator=g) + 0.5
                elif kind == 'f32':
                    t = torch.randn(count, generator=g)
                else:                                    # 'act', 'out' (a seeded start value: accumulate reads it)
                    t = torch.randn(count, generator=g).to(act)
                keep[name] = t.to(DEV).contiguous()
                return keep[name].data_ptr()

            a = cases.build(nat, mode, d['a'], alloc, 'a')
            outs = ['a.y']
            b = None
            if 'b' in d:
                b = cases.build(nat, mode, d['b'], alloc, 'b')
                cases.pair_link(a, b, alloc, 'p')
                outs.append('b.y')
            sp = nat.check(lib.dfl_conv_suggest_splits(C.addressof(a)), 'suggest')
            if sp > 1:
                M = a.N * (a.Hin * a.Win if a.scatter2x2 else a.Hout * a.Wout)
                keep['partial'] = torch.full(((2 if b is not None else 1) * sp * M * a.Ntot,), float('nan'), device=DEV)
                a.splits, a.partial = sp, keep['partial'].data_ptr()
            cfg = lib.dfl_conv_config(C.addressof(a))
            if b is not None:
                ok = lib.dfl_conv_pair_ok(C.addressof(a), C.addressof(b))
                nat.check(lib.dfl_conv2d_pair(C.addressof(a), C.addressof(b), st()), 'pair')
            else:
                ok = 0
                nat.check(lib.dfl_conv2d(C.addressof(a), st()), 'conv')
            torch.cuda.synchronize()
            rows.append(dict(mode=mode, block=d['name'], cfg=cfg, splits=sp, pair_ok=ok, sha=[sha(keep[o]) for o in outs]))
        # the eval-mode paper forward at 192 x 192, batch 1
        torch.manual_seed(5)
        net = dfl_amd.UNet(**bench.PAPER).to(DEV).eval()
        x = torch.randn(1, 1, 192, 192, generator=torch.Generator().manual_seed(6)).to(DEV)
        with torch.no_grad():
            seg, heat = net(x)
            torch.cuda.synchronize()
            plan = [p for ps in net._plans.values() for p in ps if not p.need_grad][0]
            convs = [s_ for s_ in plan.fwd.structs if isinstance(s_, nat.ConvArgs)]
            for s_ in plan.fwd.structs:
                if isinstance(s_, nat.ConvPairArgs):
                    convs += [nat.ConvArgs.from_address(s_.a), nat.ConvArgs.from_address(s_.b)]
            taken = sum(1 for s_ in convs if lib.dfl_conv_config(C.addressof(s_)) == 16 + 39)
            npairs = sum(1 for s_ in plan.fwd.structs if isinstance(s_, nat.ConvPairArgs))
        rows.append(dict(mode=mode, block='paper forward 192x192 batch 1 (latency form: %d convolutions, %d pairs)' % (taken, npairs),
                         cfg=0, splits=0, pair_ok=0, sha=[sha(seg), sha(heat)]))
    nat.check(lib.dfl_set_math_mode(0), 'dfl_set_math_mode')
    print('__ROWS__' + json.dumps(rows))


def run(libpath):
    env = dict(os.environ, DFL_LIB_OVERRIDE=os.path.abspath(libpath))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, check=True, stdout=subprocess.PIPE, timeout=420).stdout.decode()
    line = [l for l in out.splitlines() if l.startswith('__ROWS__')][0]
    return json.loads(line[len('__ROWS__'):])


def main():
    rp = run(sys.argv[1])
    rn = run(sys.argv[2])                                # (only after the first child has ended cleanly: check=True)
    bad = 0
    assert len(rp) == len(rn)
    for a, b in zip(rp, rn):
        same = a == b
        bad += 0 if same else 1
        print('%-7s %-78s cfg %3d splits %2d pair %d  %s  %s' % (a['mode'], a['block'], a['cfg'], a['splits'], a['pair_ok'],
                                                                ' '.join(h[:16] for h in a['sha']), 'same' if same else 'DIFFERS: new %s' % b))
    lat = sum(1 for a in rp if a['cfg'] == 16 + 39)
    print('RESULT: %d outputs compared (%d blocks in latency form), %s' % (sum(len(a['sha']) for a in rp), lat, 'all identical' if bad == 0 else '%d blocks differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child()
    else:
        sys.exit(main())
