#!/usr/bin/env python3
"""Training step time with each optimizer of train.py --optim, on bench.py's workload: the paper network (depth 6, 32..1024
channels, seg + 14-landmark heads) at batch 16 of synthetic 1x192x192 images, Dice + NCC loss, one step = zero_grad ->
forward -> crop -> loss -> backward -> optimizer step -> loss read one step late (train.py:405-430, as bench.py).

One network per optimizer, all built in this process from the same seeded weights; the optimizers take turns (--rounds
rounds of --steps timed steps each, so drifts of the box hit all of them alike) and the median round is reported.  Optimizers:
dfl_amd.SGD (bench.py's settings), torch.optim.Adam and dfl_amd.Adam (lr 1e-4, wd 1e-4), torch.optim.RMSprop and
dfl_amd.RMSprop (lr 1e-5, wd 1e-4, momentum 0.9).  Prints ONE JSON line: ms/step and images/s per optimizer and arithmetic.
    python tools/bench_optim.py --math bf16s,fp32 --steps 20 --warmup 5 --rounds 3      # on the GPU box"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dfl_amd  # noqa: E402
from dfl_amd import _native as nat  # noqa: E402
from dfl_amd.util import LateScalars  # noqa: E402
from bench import PAPER, MATH, synth_batch  # noqa: E402

OPTIMIZERS = {
    'dfl_amd.SGD': lambda ps: dfl_amd.SGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True),
    'torch.optim.Adam': lambda ps: torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4),
    'dfl_amd.Adam': lambda ps: dfl_amd.Adam(ps, lr=1e-4, weight_decay=1e-4),
    'torch.optim.RMSprop': lambda ps: torch.optim.RMSprop(ps, lr=1e-5, weight_decay=1e-4, momentum=0.9),
    'dfl_amd.RMSprop': lambda ps: dfl_amd.RMSprop(ps, lr=1e-5, weight_decay=1e-4, momentum=0.9),
}


def run_mode(math_name, args, dev):
    lib = nat.lib()
    nat.check(lib.dfl_set_math_mode(MATH[math_name][0]), 'dfl_set_math_mode')
    x, tseg, theat = synth_batch(args.batch, 4321, dev)
    crit = dfl_amd.DiceAndHeatMapLoss2D(skip_bg=False, heatmap_wgt=0.5)
    runs = {}
    for name in args.optim:
        torch.manual_seed(1234)
        net = dfl_amd.UNet(**PAPER).to(dev).train()
        opt = OPTIMIZERS[name](net.parameters())
        late = LateScalars(depth=1)

        def step(net=net, opt=opt, late=late):
            opt.zero_grad()
            seg, heat = net(x)
            loss = crit((dfl_amd.center_crop(seg, tseg.shape), dfl_amd.center_crop(heat, theat.shape)), (tseg, theat))
            loss.backward()
            opt.step()
            return late.push(loss)
        for _ in range(args.warmup):
            step()
        late.flush()
        runs[name] = (step, late, [])
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name in args.optim:
            step, late, times = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            late.flush()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {}
    for name in args.optim:
        ms = statistics.median(runs[name][2])
        out[name] = {'ms_per_step': round(ms, 4), 'images_per_s': round(args.batch / ms * 1e3, 1),
                     'ms_per_step_rounds': [round(t, 4) for t in runs[name][2]]}
    del runs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--math', default='bf16s,fp32', help='comma-separated arithmetics (bench.py --math names)')
    ap.add_argument('--optim', default=','.join(OPTIMIZERS), help='comma-separated subset of: ' + ', '.join(OPTIMIZERS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    args.optim = args.optim.split(',')
    for name in args.optim:
        if name not in OPTIMIZERS:
            raise SystemExit('unknown optimizer %r (choose from %s)' % (name, ', '.join(OPTIMIZERS)))
    modes = args.math.split(',')
    for m in modes:
        if m not in MATH:
            raise SystemExit('unknown --math %r' % m)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    lib = nat.lib()
    before = lib.dfl_get_math_mode()
    res = {}
    try:
        for m in modes:
            res[m] = run_mode(m, args, dev)
    finally:
        nat.check(lib.dfl_set_math_mode(before), 'dfl_set_math_mode')
    print(json.dumps({'tool': 'bench_optim', 'workload': 'paper network, batch %d, 1x192x192, Dice + NCC' % args.batch,
                      'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(dev),
                      'results': res}))


if __name__ == '__main__':
    main()
