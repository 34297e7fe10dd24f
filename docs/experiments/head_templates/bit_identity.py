#!/usr/bin/env python3
"""dfl_head_fwd / dfl_head_bwd on seeded operands at the shapes of the two kernel tests; every output goes to an .npz file.  Run once
per library in separate processes and compare byte for byte:
  DFL_LIB_OVERRIDE=<parent library> python docs/experiments/head_templates/bit_identity.py parent.npz
  python docs/experiments/head_templates/bit_identity.py new.npz
  python docs/experiments/head_templates/bit_identity.py --compare parent.npz new.npz
Cases: the 8 tuples of tests/test_gpu_kernels.py::test_heads_forward_backward (fp32 features, scratch rows, 2 x 11 x 13 pixels), the 7
of tests/test_gpu_bf16.py::test_head_backward_fused_weight_gradients (bf16 features, fused weight gradients, 3 x 37 x 29), one more
matrix-core backward call with live statistics (stat_other, zeroed stat_totals), and -- reported apart, the one route on which another
kernel runs than before -- the two cases with a w_seg that starts 4 bytes into its buffer."""
import os
import sys

import numpy as np

if sys.argv[1] == '--compare':
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), 'the two runs hold different arrays'
    bad = 0
    for part, pick in (('aligned', lambda k: not k.startswith('misaligned')), ('misaligned w_seg', lambda k: k.startswith('misaligned'))):
        keys = [k for k in sorted(a.files) if pick(k)]
        diff = [k for k in keys if a[k].tobytes() != b[k].tobytes()]
        print('%s: %d arrays of %d calls, %d differ' % (part, len(keys), len({k.split('/')[0] for k in keys}), len(diff)))
        for k in diff:
            x, y = a[k].astype(np.float64), b[k].astype(np.float64)
            print('  DIFFERS %s: largest difference %.3e (largest magnitude %.3e)' % (k, np.abs(x - y).max(), np.abs(x).max()))
        bad += len(diff)
    sys.exit(1 if bad else 0)

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import dfl_amd  # noqa: E402,F401
from dfl_amd import _native as nat  # noqa: E402

lib = nat.lib()
DEV, BF = 'cuda', torch.bfloat16
st = torch.cuda.current_stream().cuda_stream
out = {}


def keep(tag, name, t):
    t = t.detach().cpu()
    out['%s/%s' % (tag, name)] = (t.view(torch.int16) if t.dtype == BF else t).numpy()


def case(tag, NC, L, two, softmax, F_, N, H, W, bf16, w_off=0, stats=False):
    g = torch.Generator().manual_seed(1000 + 37 * NC + L + F_)
    NM = (NC + L if two else L) if L > 0 else 0
    M = N * H * W
    ldx = F_ + 8 if bf16 else F_
    x = torch.randn(M, ldx, generator=g).to(DEV)
    x = x.to(BF) if bf16 else x
    buf = torch.zeros(NC * F_ + 4, device=DEV)                       # w_seg: w_off floats into a 16-byte aligned buffer
    buf[w_off:w_off + NC * F_] = (torch.randn(NC * F_, generator=g) / 3).to(DEV)
    wseg = buf[w_off:w_off + NC * F_]
    w1 = (torch.randn(NM, F_ + NC, generator=g) / 3).to(DEV) if L > 0 else None
    w2 = (torch.randn(L, NM, generator=g) / 3).to(DEV) if (L > 0 and two) else None
    seg = torch.full((N, NC, H, W), float('nan'), device=DEV)
    heat = torch.full((N, L, H, W), float('nan'), device=DEV) if L > 0 else None
    nat.call('dfl_head_fwd', nat.HeadFwdArgs(x=x.data_ptr(), w_seg=wseg.data_ptr(), w_l1=nat.ptr(w1), w_l2=nat.ptr(w2), seg=seg.data_ptr(),
                                             heat=nat.ptr(heat), N=N, H=H, W=W, F=F_, ldx=ldx, NC=NC, NM=NM, L=L, softmax=softmax,
                                             x_bf16=int(bf16)), st)
    torch.cuda.synchronize()
    keep(tag, 'seg', seg)
    if L > 0:
        keep(tag, 'heat', heat)
    seg_in = torch.softmax(torch.randn(N, NC, H, W, generator=g), 1).to(DEV)
    dseg = torch.randn(N, NC, H, W, generator=g).to(DEV)
    dheat = torch.randn(N, L, H, W, generator=g).to(DEV) if L > 0 else None
    dx = torch.full((M, F_), float('nan'), device=DEV, dtype=BF if bf16 else torch.float32)
    a = nat.HeadBwdArgs(x=x.data_ptr(), seg=seg_in.data_ptr(), dseg=dseg.data_ptr(), dheat=nat.ptr(dheat), w_seg=wseg.data_ptr(),
                        w_l1=nat.ptr(w1), w_l2=nat.ptr(w2), dx=dx.data_ptr(), N=N, H=H, W=W, F=F_, ldx=ldx, lddx=F_, NC=NC, NM=NM, L=L,
                        softmax=softmax, x_bf16=int(bf16))
    res = {}
    if bf16:                                                         # fused weight gradients
        part = torch.full((nat.check(lib.dfl_head_wgrad_blocks(M), 'blocks') * 4096,), float('nan'), device=DEV)
        res['dw_seg'] = torch.full((NC, F_), float('nan'), device=DEV)
        if L > 0:
            res['dw_l1'] = torch.full((NM, F_ + NC), float('nan'), device=DEV)
            if two:
                res['dw_l2'] = torch.full((L, NM), float('nan'), device=DEV)
        a.wg_partial = part.data_ptr()
        a.dw_seg, a.dw_l1, a.dw_l2 = res['dw_seg'].data_ptr(), nat.ptr(res.get('dw_l1')), nat.ptr(res.get('dw_l2'))
        if stats:
            other = torch.randn(M, 32, generator=g).to(DEV).to(BF)
            res['stat_totals'] = torch.zeros(8, 2, 32, dtype=torch.float64, device=DEV)
            a.stat_other, a.ldso, a.stat_totals = other.data_ptr(), 32, res['stat_totals'].data_ptr()
    else:
        sld = lib.dfl_head_scratch_ld_for(F_, NC, NM, L)
        res['scratch'] = torch.full((M, sld), float('nan'), device=DEV)
        a.scratch, a.scratch_ld = res['scratch'].data_ptr(), sld
    nat.call('dfl_head_bwd', a, st)
    torch.cuda.synchronize()
    keep(tag, 'dx', dx)
    for k, v in res.items():
        keep(tag, k, v)


for NC, L, two, softmax, F_ in [(7, 14, True, 1, 32), (3, 14, False, 1, 8), (5, 0, True, 0, 8), (7, 14, True, 1, 4), (12, 20, True, 1, 32),
                                (16, 32, True, 1, 16), (10, 0, True, 1, 8), (3, 30, False, 0, 8)]:
    case('fp32 NC%d L%d two%d F%d' % (NC, L, two, F_), NC, L, two, softmax, F_, 2, 11, 13, False)
FUSED = [(7, 14, True, 1), (7, 0, True, 1), (5, 9, False, 1), (5, 9, True, 1), (8, 16, True, 0), (3, 0, True, 0), (2, 3, True, 1)]
for NC, L, two, softmax in FUSED:
    case('bf16 NC%d L%d two%d' % (NC, L, two), NC, L, two, softmax, 32, 3, 37, 29, True)
case('bf16 NC7 L14 two1 live statistics', 7, 14, True, 1, 32, 3, 37, 29, True, stats=True)
for NC, L, two, softmax in FUSED[:2]:
    case('misaligned bf16 NC%d L%d two%d' % (NC, L, two), NC, L, two, softmax, 32, 3, 37, 29, True, w_off=1)
np.savez(sys.argv[1], **out)
print('%d arrays of %d calls -> %s (library: %s)' % (len(out), len({k.split('/')[0] for k in out}), sys.argv[1],
                                                    os.environ.get('DFL_LIB_OVERRIDE', 'the tree\'s own')))
