#!/usr/bin/env python3
"""The convolution launches of the batch-16 paper step that a bf16 patch kernel serves (every ConvArgs of the recorded forward
and backward programs with dfl_conv_config >= 16 and bf16 operands) on seeded operands of this script's own; writes the SHA-256
of y (of `partial` under K slices), of the statistics rows / live totals and of x_out of every launch to a JSON file.  Run once
per library in separate processes and compare:
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/conv_ep_bf16/bit_identity.py parent.json
  python docs/experiments/conv_ep_bf16/bit_identity.py new.json
  python docs/experiments/conv_ep_bf16/bit_identity.py --compare parent.json new.json"""
import ctypes as C
import hashlib
import json
import os
import sys

if sys.argv[1] == '--compare':
    a, b = (json.load(open(f)) for f in sys.argv[2:4])
    bad = [k for k in a if a[k] != b.get(k)]
    fam = {}
    for k in a:
        fam[a[k]['family']] = fam.get(a[k]['family'], 0) + 1
    print('%d launches (%s), %d arrays each side; %d launches differ' % (
        len(a), ', '.join('%s %d' % kv for kv in sorted(fam.items())), sum(len(v) - 2 for v in a.values()), len(bad)))
    for k in bad:
        print('  DIFFERS: %s' % k)
    sys.exit(1 if bad or len(a) != len(b) else 0)

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat  # noqa: E402
import bench  # noqa: E402

lib = nat.lib()
nat.check(lib.dfl_set_math_mode(4), 'mode')
dev = torch.device('cuda:0')
BF = torch.bfloat16
torch.manual_seed(1234)
net = dfl_amd.UNet(**bench.PAPER).to(dev).train()
x, tseg, theat = bench.synth_batch(16, 4321, dev)
crit = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
seg, heat = net(x)
crit((dfl_amd.center_crop(seg, tseg.shape), dfl_amd.center_crop(heat, theat.shape)), (tseg, theat)).backward()
torch.cuda.synchronize()
plan = [p for ps in net._plans.values() for p in ps if p.need_grad][0]
stream = torch.cuda.current_stream().cuda_stream
sha = lambda t: hashlib.sha256(t.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def family(cfg):
    """csrc/conv_plan.hip: 16 + tile; tiles 0 ... 38 convp, 39 the latency form, 40 ... 57 convq, 58 ... 65 convn"""
    t = cfg - 16
    return 'convp' if t < 39 else 'convs' if t == 39 else 'convq' if t < 58 else 'convn'


out = {}
idx = 0
for which, prog in (('fwd', plan.fwd), ('bwd', plan.bwd)):
    for st in prog.structs:
        if not isinstance(st, nat.ConvArgs) or not (st.x_bf16 and st.y_bf16):
            continue
        cfg = lib.dfl_conv_config(C.addressof(st))
        if cfg < 16:
            continue
        a = nat.ConvArgs()
        C.memmove(C.addressof(a), C.addressof(st), C.sizeof(a))
        g = torch.Generator().manual_seed(500 + idx)
        keep = []

        def f32(n, scale=1.0, shift=0.0, rand=False):
            t = ((torch.rand(n, generator=g) if rand else torch.randn(n, generator=g)) * scale + shift).to(dev)
            keep.append(t)
            return t

        def bf(rows, ld, relu=False):
            t = torch.randn(rows, ld, generator=g)
            t = (torch.relu(t) if relu else t).to(dev).to(BF)
            keep.append(t)
            return t

        def totals(Cn, count):                            # [DFL_BN_R = 8][2][C]: row 0 carries sums of a plausible batch, the others zeros
            mean, var = torch.randn(Cn, generator=g).double() * 0.2, torch.rand(Cn, generator=g).double() + 0.5
            t = torch.zeros(8, 2, Cn, dtype=torch.float64)
            t[0, 0], t[0, 1] = mean * count, (var + mean * mean) * count
            t = t.to(dev)
            keep.append(t)
            return t

        Pin, Pout = a.N * a.Hin * a.Win, a.N * a.Hout * a.Wout
        M = Pin if a.scatter2x2 else Pout                 # GEMM rows
        Cout = a.Ntot // 4 if a.scatter2x2 else a.Ntot
        K = a.KH * a.KW * a.Cin
        a.x = bf(Pin, a.ldx).data_ptr()
        wq = (torch.randn((K + 15) // 16 * a.Ntot * 16, generator=g) / K ** 0.5).to(dev).to(BF)
        keep.append(wq)
        a.w = wq.data_ptr()
        if a.bias:
            a.bias = f32(Cout).data_ptr()
        if a.x_mode:
            a.x2 = bf(Pin, a.ldx2, relu=True).data_ptr()
            if a.in_tot:
                a.in_tot = totals(a.Cin, max(a.in_count, 1.0)).data_ptr()
                a.in_gamma = f32(a.Cin, 1.0, 0.5, rand=True).data_ptr()
                a.in_mean, a.in_invstd = f32(a.Cin, 0.2).data_ptr(), f32(a.Cin, 1.0, 0.5, rand=True).data_ptr()
            elif a.in_scale:
                coef = torch.cat([f32(a.Cin, 1.0, 0.5, rand=True), f32(a.Cin, 0.3), f32(a.Cin, 0.1)])     # A, B, C
                keep.append(coef)
                a.in_scale = coef.data_ptr()
        elif a.in_tot:
            a.in_tot = totals(a.Cin, max(a.in_count, 1.0)).data_ptr()
            a.in_gamma, a.in_beta = f32(a.Cin, 1.0, 0.5, rand=True).data_ptr(), f32(a.Cin, 0.3).data_ptr()
        elif a.in_scale:
            a.in_scale, a.in_shift = f32(a.Cin, 1.0, 0.5, rand=True).data_ptr(), f32(a.Cin, 0.3).data_ptr()
        if a.add:
            a.add = bf(max(M, Pout), a.ldadd).data_ptr()
            if a.add_scale:
                a.add_scale, a.add_shift = f32(a.Ntot, 1.0, 0.5, rand=True).data_ptr(), f32(a.Ntot, 0.2).data_ptr()
            elif a.add_tot:
                a.add_tot = totals(a.Ntot, max(a.add_count, 1.0)).data_ptr()
                a.add_gamma, a.add_beta = f32(a.Ntot, 1.0, 0.5, rand=True).data_ptr(), f32(a.Ntot, 0.2).data_ptr()
        if a.stat_other:
            a.stat_other = bf(Pout, a.ldso).data_ptr()
        if a.out_scale:
            a.out_scale, a.out_shift = f32(Cout, 1.0, 0.5, rand=True).data_ptr(), f32(Cout, 0.2).data_ptr()
        y = bf(Pout, a.ldy) if a.accumulate else torch.full((Pout, a.ldy), float('nan'), device=dev, dtype=BF)
        a.y = y.data_ptr()
        arrays = {'y': y}
        if a.splits > 1:
            part = torch.full((a.splits * M * a.Ntot,), float('nan'), device=dev)
            a.partial = part.data_ptr()
            arrays['partial'] = part
        if a.stat_partials:
            gm = nat.check(lib.dfl_conv_grid_m(C.addressof(a)), 'grid_m')
            sp = torch.full(((4 if a.scatter2x2 else 1) * gm, 2, Cout), float('nan'), device=dev)
            a.stat_partials = sp.data_ptr()
            arrays['stat_partials'] = sp
        if a.stat_totals:
            tot = torch.zeros(8, 2, a.Ntot, dtype=torch.float64, device=dev)
            a.stat_totals = tot.data_ptr()
            arrays['stat_totals'] = tot
        if a.x_out:
            xo = torch.full((Pin, a.ldxo), float('nan'), device=dev, dtype=BF)
            a.x_out = xo.data_ptr()
            arrays['x_out'] = xo
        assert lib.dfl_conv_config(C.addressof(a)) == cfg, 'the copy takes the kernel of the recorded launch'
        nat.check(lib.dfl_conv2d(C.addressof(a), stream), 'dfl_conv2d')
        torch.cuda.synchronize()
        key = '%03d %s cfg%d k%d N%d %dx%d Cin%d Ntot%d s%d splits%d relu%d add%d%d acc%d scat%d xmode%d intot%d so%d stats%d%d' % (
            idx, which, cfg, a.KH, a.N, a.Hin, a.Win, a.Cin, a.Ntot, a.stride, a.splits, a.relu, int(bool(a.add)), int(bool(a.add_tot)),
            a.accumulate, a.scatter2x2, a.x_mode, int(bool(a.in_tot)), int(bool(a.stat_other)), int(bool(a.stat_partials)), int(bool(a.stat_totals)))
        out[key] = {k: sha(v) for k, v in arrays.items()}
        out[key]['family'] = family(cfg)
        out[key]['nan_in_y'] = int(torch.isnan(y[:, :Cout].float()).sum())
        idx += 1
json.dump(out, open(sys.argv[1], 'w'), indent=1)
print('%d convolution launches hashed -> %s' % (len(out), sys.argv[1]))
