#!/usr/bin/env python3
"""The weight-gradient launches of the batch-16 step (every WgradArgs of the recorded backward program that the patch-resident
bf16 kernel serves: 21 of 3x3, 10 of 2x2, 10 of 1x1) on seeded operands of this script's own; writes the SHA-256 of dw / the
partial tiles / the bias rows of every launch to a JSON file.  Run once per library in separate processes and compare:
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/wgradp_phases/bit_identity.py parent.json
  python docs/experiments/wgradp_phases/bit_identity.py new.json;  python docs/experiments/wgradp_phases/bit_identity.py --compare parent.json new.json"""
import ctypes as C
import hashlib
import json
import os
import sys

if sys.argv[1] == '--compare':
    a, b = (json.load(open(f)) for f in sys.argv[2:4])
    bad = [k for k in a if a[k] != b.get(k)]
    print('%d launches, %d arrays each side; %d launches differ' % (len(a), sum(len(v) for v in a.values()), len(bad)))
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
out = {}
sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
idx = 0
for st in plan.bwd.structs:
    if not isinstance(st, nat.WgradArgs) or lib.dfl_wgrad_config(C.addressof(st)) < 16:
        continue
    a = nat.WgradArgs()
    C.memmove(C.addressof(a), C.addressof(st), C.sizeof(a))
    g = torch.Generator().manual_seed(100 + idx)
    M = a.N * a.Hout * a.Wout
    n = a.Cm * a.Cg * a.KH * a.KW
    gd = torch.randn(a.N * a.Hin * a.Win, a.ldg, generator=g).to(dev).to(BF)
    dd = torch.randn(M, a.ldd, generator=g).to(dev).to(BF)
    keep = [gd, dd]
    a.g, a.d = gd.data_ptr(), dd.data_ptr()
    if a.in_scale:
        sc, sh = (torch.rand(a.Cg, generator=g) + 0.5).to(dev), (torch.randn(a.Cg, generator=g) * 0.3).to(dev)
        keep += [sc, sh]
        a.in_scale, a.in_shift = sc.data_ptr(), sh.data_ptr()
    if a.d_mode:
        r = torch.relu(torch.randn(M, a.ldd2, generator=g)).to(dev).to(BF)
        coef = torch.cat([torch.rand(a.Cm, generator=g) + 0.5, torch.randn(a.Cm, generator=g) * 0.3, torch.randn(a.Cm, generator=g) * 0.1]).to(dev)
        keep += [r, coef]
        a.d2, a.coef, a.coef_tot = r.data_ptr(), coef.data_ptr(), None     # (the live-statistics form of the coefficients is derived before the loop: unchanged code)
    dw = torch.full((n,), float('nan'), device=dev)
    part = torch.full((max(a.splits, 1) * n,), float('nan'), device=dev)
    a.dw, a.partial = dw.data_ptr(), part.data_ptr()
    arrays = {'dw': dw} if a.splits == 1 else {'partial': part}
    if a.bias_partial:
        bias = torch.full((max(a.splits, 1) * a.Cm,), float('nan'), device=dev)
        a.bias_partial = bias.data_ptr()
        arrays['bias'] = bias
    nat.check(lib.dfl_conv2d_wgrad(C.addressof(a), stream), 'dfl_conv2d_wgrad')
    torch.cuda.synchronize()
    key = '%02d k%d N%d %dx%d Cg%d Cm%d s%d pad%d splits%d aff%d dmode%d bias%d' % (
        idx, a.KH, a.N, a.Hin, a.Win, a.Cg, a.Cm, a.stride, a.pad, a.splits, int(bool(a.in_scale)), a.d_mode, int(bool(a.bias_partial)))
    out[key] = {k: sha(v) for k, v in arrays.items()}
    out[key]['nan'] = int(sum(int(torch.isnan(v).sum()) for v in arrays.values()))
    idx += 1
json.dump(out, open(sys.argv[1], 'w'), indent=1)
print('%d weight-gradient launches hashed -> %s' % (len(out), sys.argv[1]))
